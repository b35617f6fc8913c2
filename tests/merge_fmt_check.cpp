// Stand-alone host check of midas_amd/csrc/merge_fmt.h (tests/test_merge_rows_host.py builds and runs it): the integer route
// to '{0:.3g}'.format(float(m) / d) against snprintf("%.3g") on the formatter's value grid, and the decimal writers against
// snprintf("%llu").  Prints the number of pairs compared; exit status 1 and the first differences on a mismatch.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../midas_amd/csrc/merge_fmt.h"

static long long n_checked = 0, n_bad = 0;

static void check(uint32_t m, uint32_t d) {
  char want[32], got[16];
  if (d == 0 || m == 0) snprintf(want, sizeof want, "0");
  else snprintf(want, sizeof want, "%.3g", (double)m / (double)d);
  const midas_fmt::Cell c = midas_fmt::freq_cell(m, d);
  for (uint32_t i = 0; i < c.len; ++i) got[i] = (char)(c.bytes >> (8 * i));
  got[c.len] = 0;
  ++n_checked;
  if (c.len > 8 || strcmp(want, got) != 0) {
    if (++n_bad <= 20) fprintf(stderr, "%u / %u: snprintf %s, merge_fmt %s\n", m, d, want, got);
  }
}

static void check_decimal(uint64_t v) {
  char want[32], got[32];
  snprintf(want, sizeof want, "%" PRIu64, v);
  const uint32_t n = midas_fmt::digits_u64(v);
  *midas_fmt::put_decimal(got, v, n) = 0;
  ++n_checked;
  if (strcmp(want, got) != 0 && ++n_bad <= 20) fprintf(stderr, "decimal %s: got %s\n", want, got);
  if (v <= 0xFFFFFFFFull) {
    const uint32_t n32 = midas_fmt::digits_u32((uint32_t)v);
    *midas_fmt::put_decimal32(got, (uint32_t)v, n32) = 0;
    if (strcmp(want, got) != 0 && ++n_bad <= 20) fprintf(stderr, "decimal32 %s: got %s\n", want, got);
  }
}

int main() {
  // every small pair
  for (uint32_t d = 0; d <= 1200; ++d)
    for (uint32_t m = 0; m <= d; ++m) check(m, d);
  // the tie families: exact three-digit ties, some representable as doubles and some not
  uint32_t fam[32];
  int nf = 0;
  for (uint32_t k = 3, p = 1000; k <= 9; ++k, p *= 10) fam[nf++] = (k == 9 ? 2000000000u : 2u * p);
  for (uint32_t k = 0, p = 1; k <= 3; ++k, p *= 10) fam[nf++] = 16u * p;
  const uint32_t more[] = {32u, 64u, 80u, 16384u, 1u << 20, 1u << 31};
  for (uint32_t v : more) fam[nf++] = v;
  for (int f = 0; f < nf; ++f) {
    const uint32_t d = fam[f], top = d < 40000u ? d : 40000u;
    for (uint32_t m = 1; m <= top; ++m) check(m, d);
  }
  // the exponent border and the extremes
  const uint32_t edge[][2] = {{99949u, 1000000000u}, {99950u, 1000000000u}, {99951u, 1000000000u}, {1u, 10000u}, {1u, 10240u},
                              {1u, 4294967294u}, {4294967294u, 4294967294u}, {4294967293u, 4294967294u}, {0u, 0u}, {5u, 0u},
                              {0u, 7u}, {9985u, 10000u}, {1999u, 2000u}, {1u, 32u}, {3u, 32u}, {1u, 4294967295u},
                              {4294967295u, 4294967295u}, {2147483647u, 4294967295u}};
  for (const auto& e : edge) check(e[0], e[1]);
  // random pairs over the whole range (a fixed generator: the run is the same every time)
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  for (int i = 0; i < 300000; ++i) {
    const int bits = 1 + (int)(next() % 32);
    uint32_t d = (uint32_t)(next() >> (64 - bits));
    if (d == 0) d = 1;
    const uint32_t m = (uint32_t)(next() % ((uint64_t)d + 1));
    check(m, d);
  }
  const uint64_t dec[] = {0ull, 9ull, 10ull, 99999ull, 100000ull, 1ull << 31, 4294967294ull, 4294967295ull, 1000000000000ull,
                          999999999999ull, 9223372036854775807ull};
  for (uint64_t v : dec) check_decimal(v);
  printf("%lld compared, %lld differ\n", n_checked, n_bad);
  return n_bad ? 1 : 0;
}
