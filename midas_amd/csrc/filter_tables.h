// keep_read's two fp64 ratio tests as exact integer thresholds: the tables the pileup kernels read, and the host function that
// fills them.  No device code: checked on the CPU by tests/cpp/filter_tables_check.cpp.
#pragma once
#include <stdint.h>

namespace midas {

constexpr int kFilterTableLen = 1025;      // kMaxLSeq + 1 (layout.h; kernels.h holds the two together)

//   min_match[a] = least x with !(100*x/float(a) < mapid)   -> keep iff (align_len - NM) >= min_match[align_len]
//   min_align[l] = least a with !(a/float(l) < aln_cov)     -> keep iff align_len >= min_align[l_seq]
struct FilterTables {
  int32_t min_match[kFilterTableLen];
  int32_t min_align[kFilterTableLen];
};

// The least passing value of a predicate that is monotone over [lo, hi] (false, then true), by bisection: lo when it passes
// there already, hi + 1 when it passes nowhere.
template <class Pass>
inline int32_t least_passing(long long lo, long long hi, Pass pass) {
  if (pass(lo)) return (int32_t)lo;
  if (!pass(hi)) return (int32_t)(hi + 1);
  while (hi - lo > 1) {      // invariant: pass(hi), !pass(lo)
    const long long mid = lo + (hi - lo) / 2;
    if (pass(mid)) hi = mid; else lo = mid;
  }
  return (int32_t)hi;
}

// The reference's own expressions (midas/run/snps.py:148, 157), evaluated in IEEE fp64 exactly as Python does, tabulated over
// every length 1..max_l a batch can contain.  Both predicates are monotone in the integer being tested.
//   min_match[a]: least x = align_len - NM in [-65535, a] with !(100*x/float(a) < mapid); a+1 if none
//   min_align[l]: least a in [1, l] with !(a/float(l) < aln_cov);                          l+1 if none
inline void build_filter_tables(double mapid, double aln_cov, int32_t max_l, FilterTables* t) {
  t->min_match[0] = 0;
  t->min_align[0] = 0;
  for (int32_t a = 1; a <= max_l && a < kFilterTableLen; ++a) {
    t->min_match[a] = least_passing(-65535, a, [&](long long x) { return !((double)(100LL * x) / (double)a < mapid); });
    t->min_align[a] = least_passing(1, a, [&](long long x) { return !((double)x / (double)a < aln_cov); });
  }
}

}  // namespace midas
