// keep_read's integer tables (midas_amd/csrc/filter_tables.h) held to the reference's own fp64 expressions: every entry is the
// least value that passes, for every length and a set of threshold pairs that reaches both end cases.
// Stand-alone: prints "ok <checks>" and returns 0, or says what failed and returns 1.
#include "filter_tables.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

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

constexpr int kMaxLSeq = kFilterTableLen - 1;

// the reference's expressions (midas/run/snps.py: keep_read), in IEEE fp64 as Python evaluates them
static bool pass_pid(long long x, int a, double mapid) { return !((double)(100LL * x) / (double)a < mapid); }
static bool pass_cov(long long x, int l, double aln_cov) { return !((double)x / (double)l < aln_cov); }

int main() {
  const double pairs[6][2] = {{94, 0.75}, {0, 0}, {100, 1}, {99.999, 1.0 / 3.0}, {-20000, 0.5}, {100.0001, 1.0001}};
  static FilterTables t;
  for (const auto& pr : pairs) {
    const double mapid = pr[0], aln_cov = pr[1];
    build_filter_tables(mapid, aln_cov, kMaxLSeq, &t);
    for (int a = 1; a <= kMaxLSeq; ++a) {
      const long long m = t.min_match[a];
      CHECK(m >= -65535 && m <= a + 1, "min_match[%d] = %lld for mapid %g", a, m, mapid);
      if (m <= a) CHECK(pass_pid(m, a, mapid), "min_match[%d] = %lld does not pass mapid %g", a, m, mapid);
      else CHECK(!pass_pid(a, a, mapid), "min_match[%d] = a + 1 although a passes mapid %g", a, mapid);
      if (m > -65535) CHECK(!pass_pid(m - 1, a, mapid), "min_match[%d] = %lld: %lld passes mapid %g as well", a, m, m - 1, mapid);
      const long long c = t.min_align[a];
      CHECK(c >= 1 && c <= a + 1, "min_align[%d] = %lld for aln_cov %g", a, c, aln_cov);
      if (c <= a) CHECK(pass_cov(c, a, aln_cov), "min_align[%d] = %lld does not pass aln_cov %g", a, c, aln_cov);
      else CHECK(!pass_cov(a, a, aln_cov), "min_align[%d] = l + 1 although l passes aln_cov %g", a, aln_cov);
      if (c > 1) CHECK(!pass_cov(c - 1, a, aln_cov), "min_align[%d] = %lld: %lld passes aln_cov %g as well", a, c, c - 1, aln_cov);
    }
    for (int a : {1, 2, 31, 151, 250, kMaxLSeq}) {      // ... and against a full linear scan
      long long m = (long long)a + 1, c = (long long)a + 1;
      for (long long x = a; x >= -65535; --x)
        if (pass_pid(x, a, mapid)) m = x;
      for (long long x = a; x >= 1; --x)
        if (pass_cov(x, a, aln_cov)) c = x;
      CHECK(t.min_match[a] == m, "min_match[%d] = %d, the scan gives %lld (mapid %g)", a, t.min_match[a], m, mapid);
      CHECK(t.min_align[a] == c, "min_align[%d] = %d, the scan gives %lld (aln_cov %g)", a, t.min_align[a], c, aln_cov);
    }
  }
  printf("ok %lld\n", n_checks);
  return 0;
}
