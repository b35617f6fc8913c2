// The host arithmetic of snp_diversity.py --rand_reads --replace_reads (sites_scan.hip, mt19937_stream.hip): numpy's legacy
// randint(0, N) takes one 32-bit MT19937 word a try, ANDs it with the smallest 2^k - 1 >= N - 1 and accepts the value when it is
// <= N - 1.  Pure functions, built by a plain C++ compiler too: tests/cpp/draw_plan_check.cpp holds them to a word-by-word model.
//   draw_mask       the mask for N
//   draw_request    raw words to ask the generator for, for a number of accepted words still missing
//   DrawLedger      which accepted words are used up, which chunk of raw words the last of them came from: the carry from one
//                   row group to the next, and where the stream stands when the call ends
#pragma once
#include <cstdint>
#include <deque>

namespace midas {

constexpr int64_t kDrawMaxReads = 2147483647ll;      // --rand_reads is capped at 2^31 - 1

// the smallest 2^k - 1 >= n - 1 (numpy's _gen_mask); n >= 1
inline uint32_t draw_mask(int64_t n) {
  uint64_t m = (uint64_t)(n - 1);
  m |= m >> 1; m |= m >> 2; m |= m >> 4; m |= m >> 8; m |= m >> 16;
  return (uint32_t)m;
}

// Raw words for `missing` accepted ones: their expected number, missing * (mask + 1) / n, and four standard deviations of the
// rejections plus 64 on top; never under 624 (a refill's worth) and never above the chunk the buffers were sized for.
inline int64_t draw_request(int64_t missing, int64_t n, int64_t chunk_cap) {
  if (missing <= 0) return 0;
  const uint64_t span = (uint64_t)draw_mask(n) + 1;
  const unsigned __int128 expect = ((unsigned __int128)(uint64_t)missing * span + (uint64_t)n - 1) / (uint64_t)n;
  uint64_t want = expect > (unsigned __int128)chunk_cap ? (uint64_t)chunk_cap : (uint64_t)expect;
  uint64_t root = 1;
  while (root * root < want) root *= 2;              // a power of two at or above the square root: above sigma
  want += 4 * root + 64;
  if (want < 624) want = 624;
  if (want > (uint64_t)chunk_cap) want = (uint64_t)chunk_cap;
  return (int64_t)want;
}

// One launch of the generator: where its raw and accepted words start in the call's stream, how many of each it made.
struct DrawChunk {
  int64_t raw_begin, raw_n, acc_begin, acc_n;
};

// The accepted words of the stream are used in order.  used: how many so far; made: how many exist.  The chunks that still
// matter are the one the last used word came from and those after it: the caller keeps the generator state each of them
// started from in a queue of its own, as long as `chunks`.
struct DrawLedger {
  std::deque<DrawChunk> chunks;
  int64_t raw_made = 0, acc_made = 0, used = 0;

  int64_t available() const { return acc_made - used; }

  // a launch made raw_n raw words of which acc_n were accepted
  void add(int64_t raw_n, int64_t acc_n) {
    chunks.push_back(DrawChunk{raw_made, raw_n, acc_made, acc_n});
    raw_made += raw_n;
    acc_made += acc_n;
  }

  // n accepted words are used up (n <= available()); chunks wholly before the last used word are forgotten
  void take(int64_t n) {
    used += n;
    while (chunks.size() > 1 && chunks.front().acc_begin + chunks.front().acc_n < used) chunks.pop_front();
  }

  // which of `chunks` the last used word lies in (-1: nothing used), and the word's index among that chunk's accepted words
  int last_chunk(int64_t* index_in_chunk) const {
    for (size_t k = 0; k < chunks.size(); ++k) {
      const DrawChunk& c = chunks[k];
      if (used > c.acc_begin && used <= c.acc_begin + c.acc_n) {
        *index_in_chunk = used - 1 - c.acc_begin;
        return (int)k;
      }
    }
    return -1;
  }
};

}  // namespace midas
