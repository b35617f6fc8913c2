// draw_plan.h against a word-by-word model: the mask is the smallest 2^k - 1 >= n - 1; a request is never 0 for a need, never
// above the chunk, at least a refill where the chunk allows, and large enough that a stream of typical yield is rarely short;
// the ledger, fed random launches and takes, names the chunk and the index of the last used word as a flat list of the accepted
// words does, never forgets a chunk that word or a later one lies in, and counts what was made and used.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <random>
#include <vector>

#include "draw_plan.h"

using namespace midas;

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);           \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main() {
  long long checks = 0;
  for (int64_t n : std::initializer_list<int64_t>{1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 100, 1000, 65536, 65537, kDrawMaxReads}) {
    const uint64_t m = draw_mask(n);
    CHECK(((m + 1) & m) == 0);                    // 2^k - 1
    CHECK(m >= (uint64_t)(n - 1));
    CHECK(m == 0 || (m >> 1) < (uint64_t)(n - 1) || n == 1);
    ++checks;
  }
  CHECK(draw_mask(1) == 0 && draw_mask(2) == 1 && draw_mask(9) == 15 && draw_mask(33) == 63 && draw_mask(kDrawMaxReads) == 0x7FFFFFFFu);
  std::mt19937_64 rng(7);
  for (int64_t n : std::initializer_list<int64_t>{2, 3, 5, 9, 33, 100, 65537, kDrawMaxReads})
    for (int64_t cap : std::initializer_list<int64_t>{64, 624, 1000, 1ll << 22})
      for (int64_t missing : std::initializer_list<int64_t>{1, 5, 623, 624, 100000, 1ll << 40}) {
        const int64_t r = draw_request(missing, n, cap);
        CHECK(r >= 1 && r <= cap);
        CHECK(r >= std::min<int64_t>(cap, 624));
        const unsigned __int128 expect = ((unsigned __int128)missing * ((uint64_t)draw_mask(n) + 1) + n - 1) / n;
        CHECK(r == cap || (unsigned __int128)r >= expect + 64);
        CHECK(draw_request(missing, n, cap) == r);
        ++checks;
      }
  CHECK(draw_request(0, 5, 1000) == 0 && draw_request(-3, 5, 1000) == 0);
  // a request's yield at the acceptance rate of the worst N (just above a power of two) is short less often than one time in 50
  {
    const int64_t n = 33, missing = 5000;
    int shortfalls = 0;
    for (int rep = 0; rep < 200; ++rep) {
      const int64_t r = draw_request(missing, n, 1ll << 22);
      int64_t got = 0;
      for (int64_t i = 0; i < r; ++i) got += (rng() & draw_mask(n)) <= (uint64_t)(n - 1);
      shortfalls += got < missing;
    }
    CHECK(shortfalls < 4);
    ++checks;
  }
  // the ledger against a flat list: (chunk, index in chunk) of every accepted word
  for (int round = 0; round < 300; ++round) {
    DrawLedger led;
    std::vector<std::pair<int64_t, int64_t>> flat;      // accepted word -> (raw_begin of its chunk, index among the chunk's accepted)
    int64_t raw = 0;
    for (int step = 0; step < 60; ++step) {
      if (rng() % 3 != 0) {
        const int64_t raw_n = 1 + (int64_t)(rng() % 50);
        const int64_t acc_n = round % 5 == 0 && rng() % 4 == 0 ? 0 : (int64_t)(rng() % (uint64_t)(raw_n + 1));
        led.add(raw_n, acc_n);
        for (int64_t i = 0; i < acc_n; ++i) flat.push_back({raw, i});
        raw += raw_n;
      } else if (led.available() > 0) {
        led.take(1 + (int64_t)(rng() % (uint64_t)led.available()));
      }
      CHECK(led.raw_made == raw && led.acc_made == (int64_t)flat.size() && led.available() == (int64_t)flat.size() - led.used);
      int64_t idx = -1;
      const int k = led.last_chunk(&idx);
      if (led.used == 0) {
        CHECK(k < 0);
      } else {
        CHECK(k >= 0 && k < (int)led.chunks.size());
        CHECK(led.chunks[(size_t)k].raw_begin == flat[(size_t)led.used - 1].first && idx == flat[(size_t)led.used - 1].second);
        CHECK(k == 0 || led.chunks.front().acc_n == 0 || led.chunks.front().acc_begin + led.chunks.front().acc_n >= led.used);
      }
      // every unused accepted word still has its chunk
      if (led.available() > 0) {
        bool found = false;
        for (const DrawChunk& c : led.chunks) found = found || c.raw_begin == flat[(size_t)led.used].first;
        CHECK(found);
      }
      ++checks;
    }
  }
  printf("ok %lld checks\n", checks);
  return 0;
}
