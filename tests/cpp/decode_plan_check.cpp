// The host arithmetic of the device BAM decode (midas_amd/csrc/decode_plan.h) held to what it promises: the regions of an inflate's
// arena, the groups and the slot size of a streamed decode, and the stitching of a record walk's chunks against a model walker.
// Stand-alone: prints "ok <checks>" and returns 0, or says what failed and returns 1.
#include "decode_plan.h"

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

// ---- layout --------------------------------------------------------------------------------------------------------------------
static void check_layout() {
  for (size_t n : {1, 2, 7, 64}) {
    for (size_t comp : {1, 255, 256, 257, 65535}) {
      for (uint32_t ulen : {0u, 1u, 65280u}) {
        size_t room = 0;
        for (size_t k = 0; k < n; ++k) room += first_pass_room(ulen);
        const size_t inflated = n * (size_t)ulen;
        const InflateLayout L(inflated, comp, n, room);
        // what each region must hold: inflated bytes (+ 64 of slack), compressed bytes (+ 512 zeroed), the block table, status and
        // match count per block, a CRC-32 per block, the match lists
        const size_t at[7] = {0, L.at_comp, L.at_blocks, L.at_status, L.at_crc, L.at_matches, L.end};
        const size_t need[6] = {inflated + 64, comp + 512, n * kInflateBlockBytes, n * 8, n * 4, room * 8};
        for (int r = 0; r < 6; ++r) {
          CHECK(at[r] % 256 == 0, "region %d of n=%zu comp=%zu ulen=%u starts at %zu", r, n, comp, ulen, at[r]);
          CHECK(at[r] + need[r] <= at[r + 1], "region %d of n=%zu comp=%zu ulen=%u: [%zu, +%zu) runs into %zu", r, n, comp, ulen, at[r], need[r], at[r + 1]);
        }
        CHECK(second_pass_room(ulen) * 8ull * 3ull >= 8ull * ulen, "second pass room of %u", ulen);
      }
    }
  }
}

// ---- plan ----------------------------------------------------------------------------------------------------------------------
static void check_plan() {
  const uint32_t ulens[3] = {0u, 1u, 65280u};
  const size_t n_jobs = 34, j_lo = 2, j_hi = 32, tail = 8;       // 30 blocks, not at either end of the table
  std::vector<InflateJob> jobs(n_jobs);
  std::mt19937 rng(17);
  uint64_t cpos = 1000, upos = 0;
  for (size_t j = 0; j < n_jobs; ++j) {
    const uint32_t ulen = ulens[rng() % 3], clen = 5 + rng() % 20000;
    jobs[j] = InflateJob{cpos + 18, upos, clen, ulen, 0u, 1u};
    cpos += clen + 26;
    upos += ulen;
  }
  for (int32_t n_ref : {0, 1, 5000}) {
    for (size_t group : {1, 4, 7, 9}) {
      const StreamPlan plan = plan_groups(jobs.data(), j_lo, j_hi, group, tail, n_ref, ~0ull);
      CHECK(plan.bad_block < 0, "group %zu: block %lld refused", group, (long long)plan.bad_block);
      CHECK(plan.groups.size() == (30 + group - 1) / group, "group %zu: %zu groups", group, plan.groups.size());
      CHECK(plan.seg_stop == jobs[j_hi - 1].upos + jobs[j_hi - 1].ulen, "group %zu: the stop is the blocks' end", group);
      for (size_t g = 0; g < plan.groups.size(); ++g) {
        const DecodeGroup& G = plan.groups[g];
        const bool last = g + 1 == plan.groups.size();
        CHECK(G.b_lo == j_lo + g * group && G.b_hi == (last ? j_hi : G.b_lo + group), "group %zu/%zu: blocks [%zu, %zu)", g, group, G.b_lo, G.b_hi);
        CHECK(G.b_ext == std::min(j_hi, G.b_hi + tail) && G.b_ext <= j_hi, "group %zu/%zu: tail to %zu", g, group, G.b_ext);
        if (last) CHECK(G.b_ext == j_hi && G.stop == plan.seg_stop, "group %zu/%zu: the last group ends with the job range", g, group);
        else CHECK(G.stop == jobs[plan.groups[g + 1].b_lo].upos && G.stop == plan.groups[g + 1].u_lo, "group %zu/%zu: stop %llu", g, group, (unsigned long long)G.stop);
        size_t room = 0, infl = 0;
        for (size_t j = G.b_lo; j < G.b_ext; ++j) { room += first_pass_room(jobs[j].ulen); infl += jobs[j].ulen; }
        CHECK(G.room == room && G.infl == infl && G.u_lo == jobs[G.b_lo].upos, "group %zu/%zu: room %zu, %zu bytes", g, group, G.room, G.infl);
        CHECK(G.comp == jobs[G.b_ext - 1].cpos + jobs[G.b_ext - 1].clen + 8 - jobs[G.b_lo].cpos, "group %zu/%zu: %zu compressed bytes", g, group, G.comp);
        // the slot holds every region of every group: the match lists of the last block too
        CHECK(G.layout().end <= plan.slot_bytes, "group %zu/%zu: its regions end at %zu, a slot is %zu", g, group, G.layout().end, plan.slot_bytes);
        CHECK(G.layout().at_matches + G.room * 8 <= plan.slot_bytes, "group %zu/%zu: match lists", g, group);
      }
    }
  }
  // a stop inside the blocks is kept; a block in front of its group's first byte is named
  const StreamPlan cut = plan_groups(jobs.data(), j_lo, j_hi, 4, tail, 1, jobs[10].upos + 1);
  CHECK(cut.seg_stop == jobs[10].upos + 1 && cut.groups.back().stop == cut.seg_stop, "a stop inside the blocks");
  for (const DecodeGroup& G : cut.groups) CHECK(G.stop <= cut.seg_stop, "no group wants more than the segment");
  std::vector<InflateJob> bad = jobs;
  bad[12].upos = 0;
  bad[12].cpos = 0;
  CHECK(plan_groups(bad.data(), j_lo, j_hi, 4, tail, 1, ~0ull).bad_block == 12, "the misplaced block is named");
}

// ---- stitch --------------------------------------------------------------------------------------------------------------------
// The model: records laid end to end; a walk from a record start p over a chunk keeps the records that start in [p, min(hi, stop))
// and ends at the first record start at or behind that (the buffer's end counts as one).
struct Model {
  std::vector<unsigned long long> starts;       // every record start, then the buffer's end
  unsigned long long total = 0;
  Model() {
    std::mt19937 rng(5);
    unsigned long long at = 0;
    bool long_one = false;
    while (at < 200000) {
      starts.push_back(at);
      const bool now = !long_one && at >= 92500;       // one record of 40 000 bytes from just below 96 KiB on: it covers the chunk [98304, 131072)
      at += now ? 40000 : 36 + rng() % 665;
      long_one = long_one || now;
    }
    starts.push_back(at);
    total = at;
  }
  unsigned long long first_at_or_behind(unsigned long long p) const { return *std::lower_bound(starts.begin(), starts.end(), p); }
  bool is_start(unsigned long long p) const { return p < total && std::binary_search(starts.begin(), starts.end() - 1, p); }
  long long count(unsigned long long lo, unsigned long long hi) const {       // record starts in [lo, hi)
    return std::lower_bound(starts.begin(), starts.end() - 1, hi) - std::lower_bound(starts.begin(), starts.end() - 1, lo);
  }
  void walk(ChunkWalk& w, size_t c, unsigned long long from) const {
    const unsigned long long top = std::min(w.hi[c], w.stop[c]);
    w.start[c] = from;
    w.bad[c] = 0;
    w.unmapped[c] = 0;
    w.first_unmapped[c] = kNoOffset;
    if (!is_start(from)) {       // (not a record: whatever the bytes there look like)
      w.kept[c] = 7; w.end[c] = from + 1234567;
      return;
    }
    w.kept[c] = (uint32_t)count(from, top);
    w.end[c] = first_at_or_behind(std::max(from, top));
    if (w.kept[c] >= 2) { w.unmapped[c] = 1; w.first_unmapped[c] = first_at_or_behind(from + 1); --w.kept[c]; }       // (its second record is unmapped)
  }
  // the walk of every chunk from its own guess: the first record start in the chunk
  ChunkWalk guessed(unsigned long long from, unsigned long long stop, bool exact) const {
    ChunkWalk w;
    w.add_segment(from, stop, total, exact);
    w.room_for_results();
    for (size_t c = 0; c < w.size(); ++c) {
      const unsigned long long guess = c == 0 && exact ? from : first_at_or_behind(w.lo[c]);
      if (guess < w.hi[c]) walk(w, c, guess);
      else { w.start[c] = kNoOffset; w.kept[c] = 99; w.unmapped[c] = 99; w.end[c] = 0; w.bad[c] = 0; }      // (no boundary found: the counts mean nothing)
    }
    return w;
  }
};

static void check_settled(const Model& m, ChunkWalk& w, const StitchResult& r, unsigned long long first, unsigned long long stop, const char* what) {
  CHECK(r.what == Stitch::settled, "%s: not settled (%d)", what, (int)r.what);
  CHECK(r.first == first, "%s: first %llu, the model's %llu", what, r.first, first);
  CHECK(r.end == m.first_at_or_behind(stop), "%s: ended at %llu, the model at %llu", what, r.end, m.first_at_or_behind(stop));
  CHECK(r.n_records + r.n_unmapped == m.count(first, stop), "%s: %lld + %lld records, the model %lld", what, r.n_records, r.n_unmapped, m.count(first, stop));
  CHECK((long long)w.count_records() == r.n_records, "%s: the chunks keep %llu records, the chain %lld", what, w.count_records(), r.n_records);
  unsigned long long at = 0;
  for (size_t c = 0; c < w.size(); ++c) {
    CHECK(w.base[c] == at, "%s: base of chunk %zu", what, c);
    at += w.kept[c];
    if (w.kept[c] || w.unmapped[c]) CHECK(m.is_start(w.start[c]), "%s: chunk %zu keeps records from %llu, no record start", what, c, w.start[c]);
  }
  if (r.n_unmapped) CHECK(m.is_start(r.first_unmapped) && r.first_unmapped > first, "%s: first unmapped at %llu", what, r.first_unmapped);
}

static void check_stitch() {
  const Model m;
  const unsigned long long stop = 190000;
  CHECK(m.total > 200000 && m.total < 245000, "the buffer is %llu bytes", m.total);
  int walked = 0, rounds = 0;
  auto again = [&](ChunkWalk& w) { return [&](size_t c, unsigned long long cur) { ++walked; m.walk(w, c, cur); return true; }; };
  {   // every guess right
    ChunkWalk w = m.guessed(0, stop, true);
    bool empty_chunk = false;
    for (size_t c = 0; c < w.size(); ++c) empty_chunk = empty_chunk || w.start[c] == kNoOffset;
    CHECK(empty_chunk, "the long record leaves a chunk with no record start");
    const StitchResult r = stitch_chunks(w, 0, w.size(), 0, &rounds, again(w));
    check_settled(m, w, r, 0, stop, "every guess right");
    CHECK(walked == 0 && rounds == 0, "every guess right: %d chunks walked again", walked);
  }
  {   // the guess of chunk 2 wrong
    ChunkWalk w = m.guessed(0, stop, true);
    m.walk(w, 2, w.start[2] + 1);
    const StitchResult r = stitch_chunks(w, 0, w.size(), 0, &rounds, again(w));
    check_settled(m, w, r, 0, stop, "chunk 2 guessed wrong");
    CHECK(walked == 1 && rounds == 1, "chunk 2 guessed wrong: %d chunks walked again", walked);
  }
  {   // an exact start in the middle, and a guessed one from the byte behind it
    const unsigned long long from = m.starts[40];
    ChunkWalk w = m.guessed(from, stop, true);
    check_settled(m, w, stitch_chunks(w, 0, w.size(), from, &rounds, again(w)), from, stop, "exact start");
    ChunkWalk v = m.guessed(from + 1, stop, false);
    check_settled(m, v, stitch_chunks(v, 0, v.size(), kNoOffset, &rounds, again(v)), m.starts[41], stop, "guessed start");
    CHECK(walked == 1, "exact / guessed start: %d chunks walked again", walked);
  }
  {   // the first two chunks find no boundary: the chain starts with the third's
    ChunkWalk w = m.guessed(1, stop, false);
    w.start[0] = w.start[1] = kNoOffset;
    const unsigned long long first = w.start[2];
    const StitchResult r = stitch_chunks(w, 0, w.size(), kNoOffset, &rounds, again(w));
    check_settled(m, w, r, first, stop, "no boundary in two chunks");
    CHECK(w.kept[0] == 0 && w.kept[1] == 0 && w.unmapped[0] == 0 && w.unmapped[1] == 0, "chunks without a boundary keep nothing");
  }
  {   // no chunk finds a boundary: nothing, and no end
    ChunkWalk w = m.guessed(1, stop, false);
    for (size_t c = 0; c < w.size(); ++c) w.start[c] = kNoOffset;
    const StitchResult r = stitch_chunks(w, 0, w.size(), kNoOffset, &rounds, again(w));
    CHECK(r.what == Stitch::settled && r.first == kNoOffset && r.end == kNoOffset && r.n_records == 0 && w.count_records() == 0, "no boundary at all");
  }
  {   // a chunk on the chain is bad
    ChunkWalk w = m.guessed(0, stop, true);
    w.bad[4] = 1;
    CHECK(stitch_chunks(w, 0, w.size(), 0, &rounds, again(w)).what == Stitch::bad_chunk, "a bad chunk on the chain");
  }
  {   // bad for a wrong guess only: walked again from the chain, it is clean
    ChunkWalk w = m.guessed(0, stop, true);
    m.walk(w, 4, w.start[4] + 2);
    w.bad[4] = 1;
    const int before = walked;
    check_settled(m, w, stitch_chunks(w, 0, w.size(), 0, &rounds, again(w)), 0, stop, "bad for a wrong guess");
    CHECK(walked == before + 1, "bad for a wrong guess: walked again once");
  }
  {   // a second walk that fails
    ChunkWalk w = m.guessed(0, stop, true);
    m.walk(w, 1, w.start[1] + 1);
    CHECK(stitch_chunks(w, 0, w.size(), 0, &rounds, [](size_t, unsigned long long) { return false; }).what == Stitch::failed, "a failed second walk");
  }
  {   // a walk that never starts where it is told to: given up, not a hang
    ChunkWalk w = m.guessed(0, stop, true);
    m.walk(w, 1, w.start[1] + 1);
    int own = 0, calls = 0;
    const StitchResult r = stitch_chunks(w, 0, w.size(), 0, &own, [&](size_t c, unsigned long long cur) { ++calls; w.start[c] = cur + 1; return true; });
    CHECK(r.what == Stitch::unsettled && calls == kStitchRounds && own == kStitchRounds + 1, "never agrees: %d calls, %d rounds", calls, own);
  }
  {   // two segments in one set of chunks share the rounds
    ChunkWalk w;
    w.add_segment(0, 60000, m.total, true);
    const size_t mid = w.size();
    w.add_segment(m.starts[200], stop, m.total, true);
    w.room_for_results();
    for (size_t c = 0; c < w.size(); ++c) m.walk(w, c, c == 0 ? 0 : (c == mid ? m.starts[200] : w.lo[c]));       // (every guess but the exact ones wrong, most likely)
    int both = 0;
    const StitchResult a = stitch_chunks(w, 0, mid, 0, &both, again(w));
    const StitchResult b = stitch_chunks(w, mid, w.size(), m.starts[200], &both, again(w));
    CHECK(a.what == Stitch::settled && b.what == Stitch::settled, "two segments settle");
    CHECK(a.n_records + a.n_unmapped == m.count(0, 60000) && a.end == m.first_at_or_behind(60000), "first segment");
    CHECK(b.n_records + b.n_unmapped == m.count(m.starts[200], stop) && b.first == m.starts[200], "second segment");
    CHECK((long long)w.count_records() == a.n_records + b.n_records && both > 0, "two segments: one count");
  }
}

int main() {
  check_layout();
  check_plan();
  check_stitch();
  printf("ok %lld checks\n", n_checks);
  return 0;
}
