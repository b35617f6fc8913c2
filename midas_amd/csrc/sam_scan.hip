// run_midas.py snps --sam on MI355X: the aligner's SAM text decoded and coordinate-sorted on the device, ending in the column form
// midas_bam_load_device leaves (small columns on the host, SEQ / QUAL / CIGAR on the device).  Replaces
// `samtools view -b | samtools sort` of midas/run/snps.py:116-120 and the open at :186.
//
//   header   the host walks the '@' lines: @SQ SN / LN in file order, everything else skipped
//   chunks   a run of bytes of the body is uploaded; it ends on its last complete line, the partial tail goes up again with
//            the next chunk.  A chunk that holds no complete line is doubled
//   index    newlines counted per 16 bytes, the library's exclusive scan, newline k's position -> ends[k] (text_rows.h)
//   pass 1   one thread a line walks the tabs once: FLAG, RNAME -> refID (sorted hashes of the @SQ names + a byte compare),
//            POS, MAPQ, l_seq, n_cigar, NM, where CIGAR / SEQ / QUAL lie in the chunk; every field rule is checked here and the
//            first bad line of the file wins (atomicMin over line << 8 | reason)
//   scans    kept flags, SEQ bytes, QUAL bytes, CIGAR ops: the library's exclusive scan -> a record's place in the columns
//   pass 2   one wave a line, lanes over bytes: SEQ letters -> 4-bit codes two a byte, QUAL - 33 (or 0xff), CIGAR text ->
//            len << 4 | op (a lane that holds an op letter ranks itself by ballot and reads its digits backwards)
//   sort     (pos + 1, index) through the library's stable radix sort, then (refID, index): equal keys keep file order
//   gather   one wave a sorted record: the small columns, the rebuilt offsets, the payload bytes in sorted order
// MIDAS_SAM_ORDER_FILE (midas_sam_load_device_order; run_midas.py genes, whose fp64 sums follow the order of the aligner's
// lines): no sort and no gather -- the columns pass 2 accumulated, chunk after chunk, ARE the result: the small ones are
// copied down, the three payload arrays are handed to the handle as they are.
// midas_sam_load_resident: the same passes and the same sort, but the gather writes the pileup kernel's own layout (layout.h
// DirectRec + payload) -- what a streamed midas_bam_load_resident leaves -- and nothing else:
//   sizes    per sorted record also its direct_payload_units and, from the byte pass 2 wrote for it ("exceptional": dense_exact
//            fails for a base), what it reserves in the side buffer; the library's scan over each
//   direct   HALF a wave a sorted record (sam_direct_kernel, shaped like bam_walk.hip's bam_direct_kernel): the CIGAR words copied,
//            SEQ + QUAL through dense::encode, the exceptional reads' raw bytes through dense::side_copy, the 16-byte record, the
//            small columns and the int64 offsets in sorted order, all to device arrays; no sorted SEQ / QUAL / CIGAR column exists.
//            The side buffer is sized exactly before the launch; only refID comes down.
// Everything a kernel reads of the text lies inside its line; everything it writes lies inside room the host sized from the
// scans' totals before the launch.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/midas_snps.h"
#include "ctx_internal.h"
#include "dense_bases.h"
#include "hostio.h"
#include "kernels.h"
#include "sam_resident_plan.h"
#include "text_rows.h"

namespace midas {
namespace {

// ---- reasons a line is refused (low byte of the error word; the host words them) ---------------------------------------------
enum : uint32_t {
  kSamShort = 1, kSamFlag, kSamRname, kSamPos, kSamMapq, kSamCigarOp, kSamCigarLen, kSamCigarMany, kSamQualLen, kSamQualChar, kSamNm
};
const char* sam_reason(uint32_t r) {
  switch (r) {
    case kSamShort: return "fewer than 11 fields";
    case kSamFlag: return "FLAG is not a decimal number in 0..65535";
    case kSamRname: return "RNAME is not among the @SQ lines";
    case kSamPos: return "POS is not a decimal number in 0..2147483647";
    case kSamMapq: return "MAPQ is not a decimal number in 0..255";
    case kSamCigarOp: return "CIGAR holds an op that is not one of MIDNSHP=X";
    case kSamCigarLen: return "a CIGAR op has no length, or one of 2^28 or more";
    case kSamCigarMany: return "CIGAR has more than 65535 ops";
    case kSamQualLen: return "QUAL and SEQ differ in length";
    case kSamQualChar: return "QUAL holds a character outside '!'..'~'";
    case kSamNm: return "NM:i: is not followed by an integer";
  }
  return "malformed";
}

constexpr uint32_t kNoQual = 0xFFFFFFFFu;
constexpr uint32_t kMaxCigarOps = 65535u;

__host__ __device__ inline uint32_t fnv1a(const char* s, uint32_t n) {
  uint32_t h = 2166136261u;
  for (uint32_t i = 0; i < n; ++i) { h ^= (uint8_t)s[i]; h *= 16777619u; }
  return h;
}

// "=ACMGRSVTWYHKDBN" -> 0..15, either case; any other byte 15.  The letters' codes are nibbles of two constants (A at bit 0).
__device__ __forceinline__ uint32_t seq_code(uint8_t c) {
  if (c == '=') return 0u;
  const uint32_t k = (uint32_t)(c | 0x20) - 'a';
  if (k >= 26u) return 15u;
  constexpr unsigned long long lo = 0xFFF3FCFFB4FFD2E1ull, hi = 0xFAF97F865Full;
  return (uint32_t)((k < 16u ? lo >> (4u * k) : hi >> (4u * (k - 16u))) & 15ull);
}

__device__ __forceinline__ int cigar_op(char c) {
  switch (c) {
    case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
    case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8;
  }
  return -1;
}

// decimal digits t[s, e) -> *v (saturating at 2^32 - 1); false: empty, or a byte that is no digit
__device__ __forceinline__ bool sam_uint(const char* t, uint32_t s, uint32_t e, uint32_t* v) {
  if (s >= e) return false;
  unsigned long long x = 0;
  for (uint32_t q = s; q < e; ++q) {
    if (!is_digit(t[q])) return false;
    x = x * 10ull + (unsigned)(t[q] - '0');
    if (x > 0xFFFFFFFFull) x = 0xFFFFFFFFull;
  }
  *v = (uint32_t)x;
  return true;
}

struct SamP {
  const char* text;              // the chunk, padded with zero bytes to a multiple of 16
  const uint32_t* ends;          // newline offsets of its lines
  long long lines;               // complete lines of the chunk
  unsigned long long line0;      // 1-based file line of the chunk's first line
  // the @SQ names: hashes sorted, the reference of every hash, the names back to back
  const uint32_t* ref_hash; const int32_t* ref_of; const uint32_t* name_off; const char* names; int32_t n_ref;
  // per line, lines + 1 entries (the last: zeros, so that a scan's last entry is the total)
  uint32_t* size[4];             // kept (0 / 1), SEQ bytes, QUAL bytes (= l_seq), CIGAR ops
  uint32_t* at[4];               // their exclusive scans
  int32_t *refid, *pos, *nm;
  uint32_t* flagmapq;            // flag | mapq << 16
  uint32_t *cig_at, *cig_len, *seq_at, *qual_at;      // where the fields lie in the chunk (qual_at kNoQual: QUAL is '*')
  unsigned long long* bad;       // min over (file line << 8 | reason)
};

// the records decoded so far, file order (kept ones only), and their payload
struct SamCols {
  int32_t *refid, *pos, *nm, *l_seq; uint32_t* n_cigar; uint8_t* mapq; uint16_t* flag;
  long long *seq_off, *qual_off, *cigar_off;
  uint8_t *seq4, *qual; uint32_t* cigar;
  uint8_t* exc;                  // (nullable; the resident decode asks for it) 1: dense_exact fails for a base of the record
};

// ---- pass 1: one thread a line ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sam_fields_kernel(SamP p) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r > p.lines) return;
  if (r == p.lines) {            // the entry behind the last line: the scans' totals end up here
#pragma unroll
    for (int k = 0; k < 4; ++k) p.size[k][r] = 0u;
    return;
  }
  const char* t = p.text;
  const uint32_t b = r == 0 ? 0u : p.ends[r - 1] + 1u;
  uint32_t e = p.ends[r];
  if (e > b && t[e - 1] == '\r') --e;
  uint32_t reason = 0;
  auto fail = [&](uint32_t why) { if (!reason) reason = why; };
  // the eleven mandatory fields: [fs[k], fe[k]); every walk stops at the line's end
  uint32_t q = b;
  uint32_t f_flag[2], f_rname[2], f_pos[2], f_mapq[2], f_cigar[2], f_seq[2], f_qual[2];
  bool is_short = false;
#define SAM_FIELD(dst, last)                                   \
  do {                                                         \
    const uint32_t s__ = q;                                    \
    while (q < e && t[q] != '\t') ++q;                         \
    dst[0] = s__; dst[1] = q;                                  \
    if (!(last)) { if (q >= e) is_short = true; else ++q; }    \
  } while (0)
  uint32_t skip[2];
  SAM_FIELD(skip, false);                       // QNAME
  if (!is_short) SAM_FIELD(f_flag, false);
  if (!is_short) SAM_FIELD(f_rname, false);
  if (!is_short) SAM_FIELD(f_pos, false);
  if (!is_short) SAM_FIELD(f_mapq, false);
  if (!is_short) SAM_FIELD(f_cigar, false);
  if (!is_short) SAM_FIELD(skip, false);        // RNEXT
  if (!is_short) SAM_FIELD(skip, false);        // PNEXT
  if (!is_short) SAM_FIELD(skip, false);        // TLEN
  if (!is_short) SAM_FIELD(f_seq, false);
  if (!is_short) SAM_FIELD(f_qual, true);
#undef SAM_FIELD
  uint32_t flag = 0, pos1 = 0, mapq = 0, n_cigar = 0, l_seq = 0, qual_at = kNoQual;
  int32_t refid = -1, nm = -1;
  if (is_short) {
    fail(kSamShort);
  } else {
    if (!sam_uint(t, f_flag[0], f_flag[1], &flag) || flag > 65535u) fail(kSamFlag);
    // RNAME
    const uint32_t rn = f_rname[1] - f_rname[0];
    if (!(rn == 1 && t[f_rname[0]] == '*')) {
      const uint32_t h = fnv1a(t + f_rname[0], rn);
      int lo = 0, hi = p.n_ref;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p.ref_hash[mid] < h) lo = mid + 1; else hi = mid;
      }
      for (; lo < p.n_ref && p.ref_hash[lo] == h && refid < 0; ++lo) {
        const int32_t k = p.ref_of[lo];
        const uint32_t n0 = p.name_off[k], n1 = p.name_off[k + 1];
        if (n1 - n0 != rn) continue;
        bool same = true;
        for (uint32_t i = 0; i < rn && same; ++i) same = p.names[n0 + i] == t[f_rname[0] + i];
        if (same) refid = k;
      }
      if (refid < 0) fail(kSamRname);
    }
    if (!sam_uint(t, f_pos[0], f_pos[1], &pos1) || pos1 > 0x7FFFFFFFu) fail(kSamPos);
    if (!sam_uint(t, f_mapq[0], f_mapq[1], &mapq) || mapq > 255u) fail(kSamMapq);
    // CIGAR: '*' or runs of digits + op letter
    if (!(f_cigar[1] - f_cigar[0] == 1 && t[f_cigar[0]] == '*')) {
      uint32_t c = f_cigar[0];
      while (c < f_cigar[1]) {
        unsigned long long len = 0;
        const uint32_t d0 = c;
        while (c < f_cigar[1] && is_digit(t[c])) {
          len = len * 10ull + (unsigned)(t[c] - '0');
          if (len > (1ull << 28)) len = 1ull << 28;
          ++c;
        }
        if (c == d0 || len >= (1ull << 28)) { fail(kSamCigarLen); break; }
        if (c >= f_cigar[1]) { fail(kSamCigarLen); break; }         // digits without an op behind them
        if (cigar_op(t[c]) < 0) { fail(kSamCigarOp); break; }
        ++c;
        if (++n_cigar > kMaxCigarOps) { fail(kSamCigarMany); break; }
      }
    }
    // SEQ, QUAL
    if (!(f_seq[1] - f_seq[0] == 1 && t[f_seq[0]] == '*')) l_seq = f_seq[1] - f_seq[0];
    if (!(f_qual[1] - f_qual[0] == 1 && t[f_qual[0]] == '*')) {
      qual_at = f_qual[0];
      if (f_qual[1] - f_qual[0] != l_seq) fail(kSamQualLen);
      else
        for (uint32_t i = f_qual[0]; i < f_qual[1]; ++i)
          if (t[i] < '!' || t[i] > '~') { fail(kSamQualChar); break; }
    }
    // the optional fields: the first NM:i:
    uint32_t o = f_qual[1];
    while (o < e && nm == -1) {
      const uint32_t s = o + 1;          // (t[o] is the tab in front of the field)
      uint32_t x = s;
      while (x < e && t[x] != '\t') ++x;
      if (x - s >= 5 && t[s] == 'N' && t[s + 1] == 'M' && t[s + 2] == ':' && t[s + 3] == 'i' && t[s + 4] == ':') {
        uint32_t d = s + 5;
        bool neg = false;
        if (d < x && (t[d] == '-' || t[d] == '+')) { neg = t[d] == '-'; ++d; }
        long long v = 0;
        bool ok = d < x;
        for (; d < x && ok; ++d) {
          if (!is_digit(t[d])) ok = false;
          else { v = v * 10 + (t[d] - '0'); if (v > (1ll << 40)) v = 1ll << 40; }
        }
        if (!ok) { fail(kSamNm); break; }
        if (neg) v = -v;
        nm = v > 0x7FFFFFFFll ? 0x7FFFFFFF : v < -0x80000000ll ? (int32_t)(-0x7FFFFFFF - 1) : (int32_t)v;
        o = e;                           // (found: a value of -1 must not start the search again)
        break;
      }
      o = x;
    }
  }
  if (reason) atomicMin(p.bad, ((p.line0 + (unsigned long long)r) << 8) | reason);
  const bool keep = !reason && refid >= 0;
  p.size[0][r] = keep ? 1u : 0u;
  p.size[1][r] = keep ? (l_seq + 1u) >> 1 : 0u;
  p.size[2][r] = keep ? l_seq : 0u;
  p.size[3][r] = keep ? n_cigar : 0u;
  p.refid[r] = refid;
  p.pos[r] = (int32_t)pos1 - 1;
  p.nm[r] = nm;
  p.flagmapq[r] = flag | mapq << 16;
  p.cig_at[r] = is_short ? 0u : f_cigar[0];
  p.cig_len[r] = is_short || n_cigar == 0 ? 0u : f_cigar[1] - f_cigar[0];
  p.seq_at[r] = is_short ? 0u : f_seq[0];
  p.qual_at[r] = qual_at;
}

// ---- pass 2: one wave a line, lanes over bytes ----------------------------------------------------------------------------------
// n_before: records kept in front of the chunk; base[3]: SEQ bytes, QUAL bytes, CIGAR ops in front of it
__global__ __launch_bounds__(256) void sam_payload_kernel(SamP p, SamCols c, long long n_before, long long base_seq, long long base_qual,
                                                          long long base_cigar) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= p.lines || !p.size[0][r]) return;           // (wave-uniform)
  const long long i = n_before + p.at[0][r];
  const uint32_t l = p.size[2][r], sb = p.size[1][r], nc = p.size[3][r];
  const long long so = base_seq + p.at[1][r], qo = base_qual + p.at[2][r], co = base_cigar + p.at[3][r];
  if (lane == 0) {
    const uint32_t fm = p.flagmapq[r];
    c.refid[i] = p.refid[r]; c.pos[i] = p.pos[r]; c.nm[i] = p.nm[r]; c.l_seq[i] = (int32_t)l; c.n_cigar[i] = nc;
    c.flag[i] = (uint16_t)(fm & 0xFFFFu); c.mapq[i] = (uint8_t)(fm >> 16);
    c.seq_off[i] = so; c.qual_off[i] = qo; c.cigar_off[i] = co;
  }
  const char* t = p.text;
  const uint32_t seq_at = p.seq_at[r], qual_at = p.qual_at[r];
  for (uint32_t j = lane; j < sb; j += 64) {
    const uint32_t hi = seq_code((uint8_t)t[seq_at + 2 * j]);
    const uint32_t lo = 2 * j + 1 < l ? seq_code((uint8_t)t[seq_at + 2 * j + 1]) : 0u;
    c.seq4[so + j] = (uint8_t)(hi << 4 | lo);
  }
  for (uint32_t j = lane; j < l; j += 64) c.qual[qo + j] = qual_at == kNoQual ? (uint8_t)0xFF : (uint8_t)(t[qual_at + j] - 33);
  if (c.exc) {       // is the read exceptional (layout.h dense_exact fails for a base; a QUAL '*' is 0xFF on every base)?  (wave-uniform)
    bool exc = false;
    for (uint32_t j = lane; j < l; j += 64)
      exc = exc || !dense_exact(seq_code((uint8_t)t[seq_at + j]), qual_at == kNoQual ? 0xFFu : (uint32_t)(uint8_t)(t[qual_at + j] - 33));
    const bool any = __ballot(exc) != 0ull;
    if (lane == 0) c.exc[i] = any ? (uint8_t)1 : (uint8_t)0;
  }
  if (nc) {
    const uint32_t cig_at = p.cig_at[r], cig_len = p.cig_len[r];
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    uint32_t done = 0;
    for (uint32_t k0 = 0; k0 < cig_len; k0 += 64) {
      const uint32_t k = k0 + lane;
      const char ch = k < cig_len ? t[cig_at + k] : '0';
      const bool is_op = k < cig_len && !is_digit(ch);
      const unsigned long long ops = __ballot(is_op);
      if (is_op) {
        uint32_t len = 0, mul = 1;
        for (uint32_t d = k; d > 0 && is_digit(t[cig_at + d - 1]); --d) {      // (leading zeros beyond ten digits multiply by whatever: they are zeros)
          len += (uint32_t)(t[cig_at + d - 1] - '0') * mul;
          mul *= 10u;
        }
        const uint32_t rank = done + (uint32_t)__popcll(ops & below);
        if (rank < nc) c.cigar[co + rank] = len << 4 | (uint32_t)cigar_op(ch);
      }
      done += (uint32_t)__popcll(ops);
    }
  }
}

// ---- sort keys, sorted sizes, gather ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sam_key_pos_kernel(const int32_t* pos, long long n, uint32_t* key, uint32_t* val) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  key[i] = (uint32_t)(pos[i] + 1);
  val[i] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void sam_key_ref_kernel(const int32_t* refid, const uint32_t* val, long long n, uint32_t* key) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) key[i] = (uint32_t)refid[val[i]];
}
// sizes of the records in sorted order, n + 1 entries (the last: zeros)
__global__ __launch_bounds__(256) void sam_sorted_sizes_kernel(const uint32_t* perm, const int32_t* l_seq, const uint32_t* n_cigar, long long n,
                                                               uint32_t* sz_seq, uint32_t* sz_qual, uint32_t* sz_cigar) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  uint32_t l = 0, nc = 0;
  if (i < n) { l = (uint32_t)l_seq[perm[i]]; nc = n_cigar[perm[i]]; }
  sz_seq[i] = (l + 1u) >> 1; sz_qual[i] = l; sz_cigar[i] = nc;
}
struct SamGatherP {
  const uint32_t* perm; long long n;
  SamCols in;                       // file order
  const uint32_t *at_seq, *at_qual, *at_cigar;       // [n + 1] scanned sizes, sorted order
  SamCols out;                      // sorted (offsets n + 1 entries)
};
__global__ __launch_bounds__(256) void sam_gather_kernel(SamGatherP g) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i > g.n) return;
  if (i == g.n) {
    if (lane == 0) { g.out.seq_off[i] = g.at_seq[i]; g.out.qual_off[i] = g.at_qual[i]; g.out.cigar_off[i] = g.at_cigar[i]; }
    return;
  }
  const uint32_t s = g.perm[i];
  const uint32_t l = (uint32_t)g.in.l_seq[s], nc = g.in.n_cigar[s], sb = (l + 1u) >> 1;
  const long long so = g.at_seq[i], qo = g.at_qual[i], co = g.at_cigar[i];
  if (lane == 0) {
    g.out.refid[i] = g.in.refid[s]; g.out.pos[i] = g.in.pos[s]; g.out.nm[i] = g.in.nm[s]; g.out.l_seq[i] = (int32_t)l;
    g.out.flag[i] = g.in.flag[s]; g.out.mapq[i] = g.in.mapq[s];
    g.out.seq_off[i] = so; g.out.qual_off[i] = qo; g.out.cigar_off[i] = co;
  }
  const long long fs = g.in.seq_off[s], fq = g.in.qual_off[s], fc = g.in.cigar_off[s];
  for (uint32_t j = lane; j < sb; j += 64) g.out.seq4[so + j] = g.in.seq4[fs + j];
  for (uint32_t j = lane; j < l; j += 64) g.out.qual[qo + j] = g.in.qual[fq + j];
  for (uint32_t j = lane; j < nc; j += 64) g.out.cigar[co + j] = g.in.cigar[fc + j];
}

// ---- the resident form: sorted sizes, then the direct layout straight from the file-order columns --------------------------------
// sam_sorted_sizes_kernel's sibling: also the record's 8-byte units in the direct layout and what it reserves in the side buffer
// (an entry, units of raw SEQ + QUAL) when pass 2 flagged it; n + 1 entries each (the last: zeros)
struct SamResidentSizes { uint32_t *seq, *qual, *cigar, *unit, *side_entries, *side_units; };
__global__ __launch_bounds__(256) void sam_resident_sizes_kernel(const uint32_t* perm, const int32_t* l_seq, const uint32_t* n_cigar, const uint8_t* exc,
                                                                 long long n, SamResidentSizes sz) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  uint32_t l = 0, nc = 0, e = 0, units = 0;
  if (i < n) { const uint32_t s = perm[i]; l = (uint32_t)l_seq[s]; nc = n_cigar[s]; e = exc[s]; units = direct_payload_units(l, nc); }
  sz.seq[i] = (l + 1u) >> 1; sz.qual[i] = l; sz.cigar[i] = nc; sz.unit[i] = units;
  sz.side_entries[i] = sam_side_entries(e); sz.side_units[i] = sam_side_units(l, e);
}
struct SamDirectP {
  const uint32_t* perm; long long n;
  SamCols in;                       // file order
  const uint32_t *at_seq, *at_qual, *at_cigar, *at_unit;       // [n + 1] scanned sizes, sorted order
  // sorted, all on the device: the records (n + 1: the sentinel), their payload, the small columns, the offsets (n + 1)
  DirectRec* rec; uint8_t* payload;
  int32_t *refid, *pos, *nm, *l_seq; uint8_t* mapq; uint16_t* flag;
  long long *seq_off, *qual_off, *cigar_off, *unit_off;
  DenseSide* side;                  // room for every flagged read (sized from the scans before the launch)
};
// HALF a wavefront per sorted record, as bam_direct_kernel: the record's CIGAR words to the 8-byte unit the scan gave it, its
// 4-bit SEQ + QUAL as the sum word and one byte a base behind them (dense_bases.h), an exceptional read's raw bytes into the side
// buffer, and by the half's first lane the 16-byte record, the small columns and the offsets.
typedef unsigned long long u64_a4 __attribute__((aligned(4)));
__global__ __launch_bounds__(256) void sam_direct_kernel(SamDirectP p) {
  const uint32_t lane = threadIdx.x & 63u, sub = lane >> 5, sl = lane & 31u;
  const long long slot = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + sub, n_slots = (long long)gridDim.x * 8;
  for (long long i = slot; i < p.n; i += n_slots) {
    const uint32_t s = p.perm[i];
    const uint32_t l = (uint32_t)p.in.l_seq[s], n_cig = p.in.n_cigar[s];
    const unsigned long long u0 = p.at_unit[i], room = ((unsigned long long)p.at_unit[i + 1] - u0) << 3;
    uint8_t* dst = p.payload + (u0 << 3);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(p.in.cigar + p.in.cigar_off[s]);
    const uint32_t nc4 = 4u * n_cig;
    for (uint32_t k = sl * 8u; k + 8u <= nc4; k += 256u) *reinterpret_cast<unsigned long long*>(dst + k) = *reinterpret_cast<const u64_a4*>(src + k);
    if (sl == 0u && (n_cig & 1u)) *reinterpret_cast<uint32_t*>(dst + nc4 - 4u) = *reinterpret_cast<const uint32_t*>(src + nc4 - 4u);
    const uint8_t* seq = p.in.seq4 + p.in.seq_off[s];
    const uint8_t* qual = p.in.qual + p.in.qual_off[s];
    const bool exc = dense::encode<32>(dst + nc4, (uint32_t)(room - nc4), seq, qual, l, (int)sl, p.side);
    if (exc) dense::side_copy<32>(p.side, (unsigned long long)i, seq, qual, l, (int)sl);
    if (sl == 0u) {
      const int32_t nm = p.in.nm[s], pos = p.in.pos[s];
      const uint32_t mapq = p.in.mapq[s];
      p.rec[i] = direct_rec(pos, l, n_cig, nm, mapq, (uint32_t)u0);
      p.refid[i] = p.in.refid[s]; p.pos[i] = pos; p.nm[i] = nm; p.l_seq[i] = (int32_t)l; p.mapq[i] = (uint8_t)mapq; p.flag[i] = p.in.flag[s];
      p.seq_off[i] = p.at_seq[i]; p.qual_off[i] = p.at_qual[i]; p.cigar_off[i] = p.at_cigar[i]; p.unit_off[i] = (long long)u0;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {       // the sentinel: where the payload ends; the offsets' last entries
    const long long n = p.n;
    p.rec[n] = direct_rec(0, 0u, 0u, 0, 0u, p.at_unit[n]);
    p.seq_off[n] = p.at_seq[n]; p.qual_off[n] = p.at_qual[n]; p.cigar_off[n] = p.at_cigar[n]; p.unit_off[n] = p.at_unit[n];
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
struct SamFile {
  const char* base = nullptr;
  size_t size = 0;
  ~SamFile() { if (base && size) munmap(const_cast<char*>(base), size); }
};

// a device array that grows by doubling and keeps what it holds
struct DevGrow {
  void* p = nullptr;
  size_t cap = 0;
  ~DevGrow() { if (p) (void)hipFree(p); }
  hipError_t need(size_t bytes, size_t keep, hipStream_t st) {
    if (bytes <= cap) return hipSuccess;
    size_t want = std::max(bytes, cap * 2);
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, want);
    if (e != hipSuccess && want > bytes) { (void)hipGetLastError(); want = bytes; e = hipMalloc(&q, want); }
    if (e != hipSuccess) return e;
    if (keep) {
      e = hipMemcpyAsync(q, p, keep, hipMemcpyDeviceToDevice, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) { (void)hipFree(q); return e; }
    }
    if (p) (void)hipFree(p);
    p = q;
    cap = want;
    return hipSuccess;
  }
  void drop() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

void device_free(void* p) { if (p) (void)hipFree(p); }

int32_t sam_err(char* err256, int32_t st, const char* fmt, const char* a, long long b, const char* c = "") {
  if (err256) snprintf(err256, 256, fmt, a, b, c);
  return st;
}

// the '@' lines: references from @SQ; *body = offset of the first line that is no header line, *n_lines = header lines
int32_t sam_header(const SamFile& f, const char* path, std::vector<std::string>& names, std::vector<int64_t>& lens, size_t* body,
                   long long* n_lines, char* err256) {
  size_t at = 0;
  long long line = 0;
  std::unordered_set<std::string> seen_names;
  while (at < f.size && f.base[at] == '@') {
    ++line;
    const char* nl = static_cast<const char*>(memchr(f.base + at, '\n', f.size - at));
    const size_t next = nl ? (size_t)(nl - f.base) + 1 : f.size;
    size_t e = nl ? (size_t)(nl - f.base) : f.size;
    if (e > at && f.base[e - 1] == '\r') --e;
    if (e - at >= 3 && f.base[at + 1] == 'S' && f.base[at + 2] == 'Q' && (e - at == 3 || f.base[at + 3] == '\t')) {
      // the first SN: and the first LN: of the line count; a later one is not looked at
      std::string sn;
      bool seen_sn = false, seen_ln = false, has_ln = false;
      int64_t ln = 0;
      size_t q = at + 3;
      while (q < e) {
        const size_t s = q + 1;
        size_t x = s;
        while (x < e && f.base[x] != '\t') ++x;
        if (x - s >= 3 && f.base[s + 2] == ':') {
          if (f.base[s] == 'S' && f.base[s + 1] == 'N' && !seen_sn) { seen_sn = true; sn.assign(f.base + s + 3, x - s - 3); }
          if (f.base[s] == 'L' && f.base[s + 1] == 'N' && !seen_ln) {
            seen_ln = true;
            has_ln = x > s + 3;
            for (size_t d = s + 3; d < x && has_ln; ++d) {
              if (f.base[d] < '0' || f.base[d] > '9') has_ln = false;
              else { ln = ln * 10 + (f.base[d] - '0'); if (ln > 0x7FFFFFFFll) has_ln = false; }
            }
          }
        }
        q = x;
      }
      if (sn.empty() || !has_ln) return sam_err(err256, MIDAS_SNPS_ERR_BAD_LAYOUT, "%s: line %lld: @SQ without a usable SN: or LN:", path, line);
      if (!seen_names.insert(sn).second) return sam_err(err256, MIDAS_SNPS_ERR_BAD_LAYOUT, "%s: line %lld: @SQ repeats SN:%s", path, line, sn.c_str());
      names.push_back(sn);
      lens.push_back(ln);
    }
    at = next;
  }
  *body = at;
  *n_lines = line;
  if (names.empty() && at < f.size)
    return sam_err(err256, MIDAS_SNPS_ERR_BAD_LAYOUT, "%s: line %lld: a record in front of any @SQ line", path, line + 1);
  return MIDAS_SNPS_OK;
}

}  // namespace
}  // namespace midas

using namespace midas;

extern "C" int32_t midas_sam_decode_timing(const midas_snps_ctx* ctx, float* out_ms8) {
  if (!ctx || !out_ms8) return MIDAS_SNPS_ERR_INVALID_ARG;
  for (int k = 0; k < 8; ++k) out_ms8[k] = ctx->sam_ms[k];
  return MIDAS_SNPS_OK;
}

namespace {

// the three payload arrays of a file-order decode: separate allocations, freed together when the handle closes
struct SamPayloadOwner { void* p[3]; };
void sam_payload_free(void* o) {
  SamPayloadOwner* w = static_cast<SamPayloadOwner*>(o);
  if (!w) return;
  for (void* q : w->p) if (q) (void)hipFree(q);
  delete w;
}

// resident (coordinate order only): the handle of midas_sam_load_resident instead of the columns
int32_t sam_load(const char* path, midas_snps_ctx* ctx, int32_t order, bool resident, midas_bam** out, int64_t* n_reads, int64_t* seq_bytes,
                 int64_t* qual_bytes, int64_t* n_cigar, char* err256) {
  if (!ctx || !path || !out || (order != MIDAS_SAM_ORDER_COORDINATE && order != MIDAS_SAM_ORDER_FILE)) return MIDAS_SNPS_ERR_INVALID_ARG;
  const bool file_order = order == MIDAS_SAM_ORDER_FILE;
  if (resident && file_order) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  if (err256) err256[0] = 0;
  using clock = std::chrono::steady_clock;
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // map + header, upload, index, pass 1, scans, pass 2, sort + gather, columns down
  auto t0 = clock::now();
  auto lap = [&](int slot) {
    const auto t1 = clock::now();
    ms[slot] += std::chrono::duration<float, std::milli>(t1 - t0).count();
    t0 = t1;
  };
  // ---- map, header ------------------------------------------------------------------------------------------------------------
  SamFile f;
  {
    const int fd = ::open(path, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) {
      if (fd >= 0) ::close(fd);
      return sam_err(err256, MIDAS_SNPS_ERR_INVALID_ARG, "%s cannot be read", path, 0);
    }
    f.size = (size_t)sb.st_size;
    if (f.size) {
      void* m = mmap(nullptr, f.size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (m == MAP_FAILED) { ::close(fd); f.size = 0; return sam_err(err256, MIDAS_SNPS_ERR_INVALID_ARG, "%s cannot be mapped", path, 0); }
      f.base = static_cast<const char*>(m);
    }
    ::close(fd);
  }
  std::vector<std::string> names;
  std::vector<int64_t> lens;
  size_t body = 0;
  long long header_lines = 0;
  {
    const int32_t st = sam_header(f, path, names, lens, &body, &header_lines, err256);
    if (st != MIDAS_SNPS_OK) return st;
  }
  const int32_t n_ref = (int32_t)names.size();
  lap(0);

  auto hip_err = [&](hipError_t e, const char* what) {
    if (err256) snprintf(err256, 256, "SAM decode: %s: %s", what, hipGetErrorString(e));
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? MIDAS_SNPS_ERR_OUT_OF_MEMORY : MIDAS_SNPS_ERR_HIP;
  };
#define SAM_TRY(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return hip_err(e__, #call); } while (0)
  std::lock_guard<std::mutex> guard(ctx->device_mutex);
  SAM_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SsBufs dev;

  // ---- the @SQ names on the device: hashes sorted, the names back to back ---------------------------------------------------------
  uint32_t *d_ref_hash = nullptr, *d_name_off = nullptr;
  int32_t* d_ref_of = nullptr;
  char* d_names = nullptr;
  {
    std::vector<std::pair<uint32_t, int32_t>> hk((size_t)n_ref);
    std::vector<uint32_t> noff((size_t)n_ref + 1, 0u);
    std::string pool;
    for (int32_t k = 0; k < n_ref; ++k) {
      hk[(size_t)k] = {fnv1a(names[(size_t)k].data(), (uint32_t)names[(size_t)k].size()), k};
      pool += names[(size_t)k];
      noff[(size_t)k + 1] = (uint32_t)pool.size();
    }
    std::sort(hk.begin(), hk.end());
    std::vector<uint32_t> hs((size_t)n_ref);
    std::vector<int32_t> of((size_t)n_ref);
    for (int32_t k = 0; k < n_ref; ++k) { hs[(size_t)k] = hk[(size_t)k].first; of[(size_t)k] = hk[(size_t)k].second; }
    SAM_TRY(dev.get(&d_ref_hash, (size_t)n_ref * 4));
    SAM_TRY(dev.get(&d_ref_of, (size_t)n_ref * 4));
    SAM_TRY(dev.get(&d_name_off, ((size_t)n_ref + 1) * 4));
    SAM_TRY(dev.get(&d_names, pool.size()));
    if (n_ref) {
      SAM_TRY(hipMemcpyAsync(d_ref_hash, hs.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, st));
      SAM_TRY(hipMemcpyAsync(d_ref_of, of.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, st));
      SAM_TRY(hipMemcpyAsync(d_names, pool.data(), pool.size(), hipMemcpyHostToDevice, st));
    }
    SAM_TRY(hipMemcpyAsync(d_name_off, noff.data(), ((size_t)n_ref + 1) * 4, hipMemcpyHostToDevice, st));
    SAM_TRY(hipStreamSynchronize(st));          // (the vectors go out of scope)
  }

  // ---- chunk size: the caller's (MIDAS_SNPS_SAM_CHUNK_BYTES) or an eighth of the free device memory ---------------------------------
  constexpr long long kChunkMax = 1ll << 30;      // newline offsets are 32-bit
  const long long text_bytes = (long long)(f.size - body);
  long long chunk_bytes = 0;
  if (const char* e = getenv("MIDAS_SNPS_SAM_CHUNK_BYTES")) chunk_bytes = strtoll(e, nullptr, 10);
  if (chunk_bytes <= 0) {
    size_t free_b = 0, total_b = 0;
    SAM_TRY(hipMemGetInfo(&free_b, &total_b));
    chunk_bytes = std::max<long long>(1 << 20, (long long)(free_b / 8));
  }
  chunk_bytes = std::min(std::max<long long>(chunk_bytes, 16), kChunkMax);
  chunk_bytes = std::min(chunk_bytes, std::max<long long>(16, text_bytes + 1));

  DevGrow g_text, g_counts, g_scratch, g_ends, g_line;      // the chunk: text, newline counts, scan sums, line ends, per-line arrays
  DevGrow g_refid, g_pos, g_nm, g_lseq, g_ncig, g_mapq, g_flag, g_soff, g_qoff, g_coff, g_seq, g_qual, g_cigar;   // the records so far
  DevGrow g_exc;                                                                                                    // (resident: their "exceptional" bytes)
  unsigned long long* d_bad = nullptr;
  SAM_TRY(dev.get(&d_bad, 8));
  SAM_TRY(hipMemsetAsync(d_bad, 0xFF, 8, st));
  long long n = 0, tot_seq = 0, tot_qual = 0, tot_cigar = 0;     // kept records and their payload so far
  long long at = 0, lines_before = 0;
  SamCols cols{};

  while (at < text_bytes) {
    // ---- upload -----------------------------------------------------------------------------------------------------------------
    const long long left = text_bytes - at;
    long long cb = std::min(left, chunk_bytes);
    const bool at_eof = cb == left;
    const size_t padded = ((size_t)cb + 1 + 15) / 16 * 16;
    SAM_TRY(g_text.need(padded, 0, st));
    SAM_TRY(g_counts.need(padded / 16 * 4, 0, st));
    SAM_TRY(g_scratch.need(scan_scratch_words((long long)(padded / 16) + 1) * 4, 0, st));
    char* d_text = static_cast<char*>(g_text.p);
    uint32_t* d_counts = static_cast<uint32_t*>(g_counts.p);
    SAM_TRY(hipMemcpyAsync(d_text, f.base + body + at, (size_t)cb, hipMemcpyHostToDevice, st));
    long long nb = cb;
    if (at_eof && f.base[body + at + cb - 1] != '\n') {      // the last line has no terminator: it is a line all the same
      const char nl = '\n';
      SAM_TRY(hipMemcpyAsync(d_text + nb, &nl, 1, hipMemcpyHostToDevice, st));
      ++nb;
    }
    const long long n16 = (nb + 15) / 16;
    if (n16 * 16 > nb) SAM_TRY(hipMemsetAsync(d_text + nb, 0, (size_t)(n16 * 16 - nb), st));
    SAM_TRY(hipStreamSynchronize(st));
    lap(1);
    // ---- index ------------------------------------------------------------------------------------------------------------------
    hipLaunchKernelGGL(ss_count_kernel, dim3(nblocks(n16, 256)), dim3(256), 0, st, (const uint4*)d_text, n16, d_counts);
    SAM_TRY(hipGetLastError());
    uint32_t last_count = 0, last_prefix = 0;
    SAM_TRY(hipMemcpyAsync(&last_count, d_counts + n16 - 1, 4, hipMemcpyDeviceToHost, st));
    SAM_TRY(launch_scan_u32(d_counts, d_counts, n16, static_cast<uint32_t*>(g_scratch.p), st));
    SAM_TRY(hipMemcpyAsync(&last_prefix, d_counts + n16 - 1, 4, hipMemcpyDeviceToHost, st));
    SAM_TRY(hipStreamSynchronize(st));
    const long long lines = (long long)last_count + last_prefix;
    if (lines == 0) {           // not one complete line in the chunk: a longer one
      lap(2);
      if (at_eof) break;        // (cannot happen: the last chunk ends in a newline)
      if (chunk_bytes >= kChunkMax) return sam_err(err256, MIDAS_SNPS_ERR_UNSUPPORTED, "%s: line %lld is longer than 1 GiB", path, header_lines + lines_before + 1);
      chunk_bytes = std::min(kChunkMax, chunk_bytes * 2);
      continue;
    }
    SAM_TRY(g_ends.need((size_t)lines * 4, 0, st));
    uint32_t* d_ends = static_cast<uint32_t*>(g_ends.p);
    hipLaunchKernelGGL(ss_ends_kernel, dim3(nblocks(n16, 256)), dim3(256), 0, st, (const uint4*)d_text, n16, d_counts, (uint32_t)lines, d_ends);
    SAM_TRY(hipGetLastError());
    uint32_t last_end = 0;
    SAM_TRY(hipMemcpyAsync(&last_end, d_ends + lines - 1, 4, hipMemcpyDeviceToHost, st));
    SAM_TRY(hipStreamSynchronize(st));
    lap(2);
    // ---- pass 1 -----------------------------------------------------------------------------------------------------------------
    const size_t L1 = (size_t)lines + 1;
    SAM_TRY(g_line.need(L1 * 4 * 16, 0, st));
    SAM_TRY(g_scratch.need(scan_scratch_words((long long)L1) * 4, 0, st));
    uint32_t* lw = static_cast<uint32_t*>(g_line.p);
    SamP p{};
    p.text = d_text; p.ends = d_ends; p.lines = lines; p.line0 = (unsigned long long)(header_lines + lines_before + 1);
    p.ref_hash = d_ref_hash; p.ref_of = d_ref_of; p.name_off = d_name_off; p.names = d_names; p.n_ref = n_ref;
    for (int k = 0; k < 4; ++k) { p.size[k] = lw + (size_t)k * L1; p.at[k] = lw + (size_t)(4 + k) * L1; }
    p.refid = reinterpret_cast<int32_t*>(lw + 8 * L1); p.pos = reinterpret_cast<int32_t*>(lw + 9 * L1); p.nm = reinterpret_cast<int32_t*>(lw + 10 * L1);
    p.flagmapq = lw + 11 * L1; p.cig_at = lw + 12 * L1; p.cig_len = lw + 13 * L1; p.seq_at = lw + 14 * L1; p.qual_at = lw + 15 * L1;
    p.bad = d_bad;
    hipLaunchKernelGGL(sam_fields_kernel, dim3(nblocks((long long)L1, 256)), dim3(256), 0, st, p);
    SAM_TRY(hipGetLastError());
    unsigned long long bad = ~0ull;
    SAM_TRY(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st));
    SAM_TRY(hipStreamSynchronize(st));
    lap(3);
    if (bad != ~0ull)
      return sam_err(err256, MIDAS_SNPS_ERR_BAD_LAYOUT, "%s: line %lld: %s", path, (long long)(bad >> 8), sam_reason((uint32_t)(bad & 0xFFu)));
    // ---- scans ------------------------------------------------------------------------------------------------------------------
    uint32_t tot[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k) SAM_TRY(launch_scan_u32(p.size[k], p.at[k], (long long)L1, static_cast<uint32_t*>(g_scratch.p), st));
    // (the four totals lie L1 words apart: one strided copy)
    SAM_TRY(hipMemcpy2DAsync(tot, 4, p.at[0] + lines, L1 * 4, 4, 4, hipMemcpyDeviceToHost, st));
    SAM_TRY(hipStreamSynchronize(st));
    lap(4);
    // ---- pass 2: room for the chunk's records first --------------------------------------------------------------------------------
    const size_t n2 = (size_t)n + tot[0];
    SAM_TRY(g_refid.need(n2 * 4, (size_t)n * 4, st)); SAM_TRY(g_pos.need(n2 * 4, (size_t)n * 4, st)); SAM_TRY(g_nm.need(n2 * 4, (size_t)n * 4, st));
    SAM_TRY(g_lseq.need(n2 * 4, (size_t)n * 4, st)); SAM_TRY(g_ncig.need(n2 * 4, (size_t)n * 4, st)); SAM_TRY(g_mapq.need(n2, (size_t)n, st));
    SAM_TRY(g_flag.need(n2 * 2, (size_t)n * 2, st)); SAM_TRY(g_soff.need(n2 * 8, (size_t)n * 8, st)); SAM_TRY(g_qoff.need(n2 * 8, (size_t)n * 8, st));
    SAM_TRY(g_coff.need(n2 * 8, (size_t)n * 8, st));
    // (64 bytes of room behind each: a file-order decode keeps these arrays, and zeroes that room as the sorted one does)
    SAM_TRY(g_seq.need((size_t)tot_seq + tot[1] + 64, (size_t)tot_seq, st)); SAM_TRY(g_qual.need((size_t)tot_qual + tot[2] + 64, (size_t)tot_qual, st));
    SAM_TRY(g_cigar.need(((size_t)tot_cigar + tot[3]) * 4 + 64, (size_t)tot_cigar * 4, st));
    cols.refid = static_cast<int32_t*>(g_refid.p); cols.pos = static_cast<int32_t*>(g_pos.p); cols.nm = static_cast<int32_t*>(g_nm.p);
    cols.l_seq = static_cast<int32_t*>(g_lseq.p); cols.n_cigar = static_cast<uint32_t*>(g_ncig.p); cols.mapq = static_cast<uint8_t*>(g_mapq.p);
    cols.flag = static_cast<uint16_t*>(g_flag.p); cols.seq_off = static_cast<long long*>(g_soff.p); cols.qual_off = static_cast<long long*>(g_qoff.p);
    cols.cigar_off = static_cast<long long*>(g_coff.p); cols.seq4 = static_cast<uint8_t*>(g_seq.p); cols.qual = static_cast<uint8_t*>(g_qual.p);
    cols.cigar = static_cast<uint32_t*>(g_cigar.p);
    if (resident) SAM_TRY(g_exc.need(n2, (size_t)n, st));
    cols.exc = static_cast<uint8_t*>(g_exc.p);
    if (tot[0]) {
      hipLaunchKernelGGL(sam_payload_kernel, dim3(nblocks(lines, 4)), dim3(256), 0, st, p, cols, n, tot_seq, tot_qual, tot_cigar);
      SAM_TRY(hipGetLastError());
      SAM_TRY(hipStreamSynchronize(st));
    }
    lap(5);
    n += tot[0]; tot_seq += tot[1]; tot_qual += tot[2]; tot_cigar += tot[3];
    if (n > kSamMaxRecords) return sam_err(err256, MIDAS_SNPS_ERR_UNSUPPORTED, "%s: more than 2 * 10^9 records (%lld): decode it in parts", path, n);
    lines_before += lines;
    at += (long long)last_end + 1;           // (a final line without '\n': one past the text, and the loop ends)
  }
  if (file_order) {
    // ---- file order: the accumulated columns are the result ------------------------------------------------------------------------
    std::unique_ptr<midas_bam, void (*)(midas_bam*)> b(bam_new_columns_handle(path, names, lens), midas_bam_close);
    HostColumns hc{};
    if (!b || !bam_alloc_host_columns(b.get(), n, &hc)) return sam_err(err256, MIDAS_SNPS_ERR_OUT_OF_MEMORY, "%s: out of host memory for %lld records", path, n);
    SAM_TRY(g_seq.need(64, 0, st)); SAM_TRY(g_qual.need(64, 0, st)); SAM_TRY(g_cigar.need(64, 0, st));      // (no record at all: the room alone)
    SAM_TRY(hipMemsetAsync(static_cast<uint8_t*>(g_seq.p) + tot_seq, 0, 64, st));
    SAM_TRY(hipMemsetAsync(static_cast<uint8_t*>(g_qual.p) + tot_qual, 0, 64, st));
    SAM_TRY(hipMemsetAsync(static_cast<uint8_t*>(g_cigar.p) + (size_t)tot_cigar * 4, 0, 64, st));
    if (n > 0) {
      const size_t nn = (size_t)n;
      SAM_TRY(hipMemcpyAsync(hc.refid, cols.refid, nn * 4, hipMemcpyDeviceToHost, st)); SAM_TRY(hipMemcpyAsync(hc.pos, cols.pos, nn * 4, hipMemcpyDeviceToHost, st));
      SAM_TRY(hipMemcpyAsync(hc.nm, cols.nm, nn * 4, hipMemcpyDeviceToHost, st)); SAM_TRY(hipMemcpyAsync(hc.l_seq, cols.l_seq, nn * 4, hipMemcpyDeviceToHost, st));
      SAM_TRY(hipMemcpyAsync(hc.flag, cols.flag, nn * 2, hipMemcpyDeviceToHost, st)); SAM_TRY(hipMemcpyAsync(hc.mapq, cols.mapq, nn, hipMemcpyDeviceToHost, st));
      SAM_TRY(hipMemcpyAsync(hc.seq_off, cols.seq_off, nn * 8, hipMemcpyDeviceToHost, st)); SAM_TRY(hipMemcpyAsync(hc.qual_off, cols.qual_off, nn * 8, hipMemcpyDeviceToHost, st));
      SAM_TRY(hipMemcpyAsync(hc.cigar_off, cols.cigar_off, nn * 8, hipMemcpyDeviceToHost, st));
    }
    SAM_TRY(hipStreamSynchronize(st));
    hc.seq_off[n] = tot_seq; hc.qual_off[n] = tot_qual; hc.cigar_off[n] = tot_cigar;
    lap(7);
    SamPayloadOwner* own = new (std::nothrow) SamPayloadOwner{{g_seq.p, g_qual.p, g_cigar.p}};
    if (!own) return sam_err(err256, MIDAS_SNPS_ERR_OUT_OF_MEMORY, "%s: out of host memory for %lld records", path, n);
    bam_set_device_payload(b.get(), g_seq.p, g_qual.p, g_cigar.p, own, sam_payload_free);
    g_seq.p = g_qual.p = g_cigar.p = nullptr;
    bam_columns_ready(b.get(), n);
    if (n_reads) *n_reads = n;
    if (seq_bytes) *seq_bytes = tot_seq;
    if (qual_bytes) *qual_bytes = tot_qual;
    if (n_cigar) *n_cigar = tot_cigar;
    for (int k = 0; k < 8; ++k) ctx->sam_ms[k] = ms[k];
    *out = b.release();
    return MIDAS_SNPS_OK;
  }
  if (tot_qual >= kSamMaxQualBytes)
    return sam_err(err256, MIDAS_SNPS_ERR_UNSUPPORTED, "%s: %lld bytes of QUAL: the SAM decode's sorted offsets address 4 GiB of them", path, tot_qual);
  if (tot_cigar >= kSamMaxCigarOps)
    return sam_err(err256, MIDAS_SNPS_ERR_UNSUPPORTED, "%s: %lld CIGAR ops: the SAM decode's sorted offsets address 2^32 of them", path, tot_cigar);

  // ---- sort + gather ----------------------------------------------------------------------------------------------------------------
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t n1 = (size_t)n + 1;
  // the n > 0 records' order: (pos + 1, index), then (refID, index) through the stable sort -> *perm; *scratch also holds a scan of n + 1
  auto sort_records = [&](uint32_t** perm, uint32_t** scratch_out) -> int32_t {
    uint32_t *ka = nullptr, *va = nullptr, *kb = nullptr, *vb = nullptr, *scratch = nullptr;
    SAM_TRY(dev.get(&ka, (size_t)n * 4)); SAM_TRY(dev.get(&va, (size_t)n * 4)); SAM_TRY(dev.get(&kb, (size_t)n * 4)); SAM_TRY(dev.get(&vb, (size_t)n * 4));
    SAM_TRY(dev.get(&scratch, std::max(sort_scratch_words(n), scan_scratch_words((long long)n1)) * 4));
    hipLaunchKernelGGL(sam_key_pos_kernel, dim3(nblocks(n, 256)), dim3(256), 0, st, cols.pos, n, ka, va);
    SAM_TRY(hipGetLastError());
    uint32_t *ks = nullptr, *vs = nullptr;
    SAM_TRY(launch_sort_pairs_u32(ka, va, kb, vb, n, 32, scratch, st, &ks, &vs));
    if (n_ref > 1) {
      int bits = 1;
      while ((1ll << bits) < n_ref) ++bits;
      uint32_t* ko = ks == ka ? kb : ka;
      uint32_t* vo = vs == va ? vb : va;
      hipLaunchKernelGGL(sam_key_ref_kernel, dim3(nblocks(n, 256)), dim3(256), 0, st, cols.refid, vs, n, ks);
      SAM_TRY(hipGetLastError());
      SAM_TRY(launch_sort_pairs_u32(ks, vs, ko, vo, n, bits, scratch, st, &ks, &vs));
    }
    *perm = vs;
    *scratch_out = scratch;
    return MIDAS_SNPS_OK;
  };
  if (resident) {
    // ---- the direct layout from the file-order columns: sizes, scans, the result's room, ONE gather ----------------------------------
    uint32_t *perm = nullptr, *scratch = nullptr, *sz = nullptr;
    uint32_t down3[3] = {0, 0, 0};        // the scans' totals: payload units (their low 32 bits), side entries, side units
    if (n > 0) {
      const int32_t sst = sort_records(&perm, &scratch);
      if (sst != MIDAS_SNPS_OK) return sst;
      SAM_TRY(dev.get(&sz, 12 * n1 * 4));
      const SamResidentSizes zs{sz, sz + n1, sz + 2 * n1, sz + 3 * n1, sz + 4 * n1, sz + 5 * n1};
      hipLaunchKernelGGL(sam_resident_sizes_kernel, dim3(nblocks((long long)n1, 256)), dim3(256), 0, st, perm, cols.l_seq, cols.n_cigar, cols.exc, n, zs);
      SAM_TRY(hipGetLastError());
      for (int k = 0; k < 6; ++k) SAM_TRY(launch_scan_u32(sz + (size_t)k * n1, sz + (size_t)(6 + k) * n1, (long long)n1, scratch, st));
      // (the three totals lie n1 words apart: one strided copy)
      SAM_TRY(hipMemcpy2DAsync(down3, 4, sz + (size_t)9 * n1 + (size_t)n, n1 * 4, 4, 3, hipMemcpyDeviceToHost, st));
      SAM_TRY(hipStreamSynchronize(st));
    }
    const unsigned long long units = sam_units_total(sam_units_range(n, tot_qual, tot_cigar), down3[0]);
    if (units == kSamUnitsUnknown || sam_side_units_bound(n, tot_qual) > kDenseSideMaxField)
      return sam_err(err256, MIDAS_SNPS_ERR_HIP, "%s: the direct layout's size does not follow from its %lld records' columns", path, n);
    if (!sam_payload_fits(units))
      return sam_err(err256, MIDAS_SNPS_ERR_UNSUPPORTED, "%s: %lld bytes of read payload exceed the 32 GiB the direct layout addresses", path, (long long)(units * 8ull));
    const SamSideSize side_size = sam_side_size(down3[1], down3[2]);
    // the result: the records' arrays in one allocation (rec, refid, pos, nm, l_seq, mapq, flag, four offset columns), the payload, the side buffer
    size_t col_at[11], col_bytes = 0;
    for (int k = 0; k < 11; ++k) { col_at[k] = col_bytes; col_bytes += up((n1 + 1) * (k == 0 ? 16 : (k <= 4 ? 4 : (k == 5 ? 1 : (k == 6 ? 2 : 8))))); }
    std::unique_ptr<SamPayloadOwner, void (*)(void*)> res_own(new (std::nothrow) SamPayloadOwner{{nullptr, nullptr, nullptr}}, sam_payload_free);
    if (!res_own) return sam_err(err256, MIDAS_SNPS_ERR_OUT_OF_MEMORY, "%s: out of host memory for %lld records", path, n);
    SAM_TRY(hipMalloc(&res_own->p[0], col_bytes));
    SAM_TRY(hipMalloc(&res_own->p[1], (size_t)units * 8 + 64));
    SAM_TRY(hipMalloc(&res_own->p[2], (size_t)side_size.alloc_bytes));
    uint8_t* cb = static_cast<uint8_t*>(res_own->p[0]);
    uint8_t* pay = static_cast<uint8_t*>(res_own->p[1]);
    DenseSide* d_side = static_cast<DenseSide*>(res_own->p[2]);
    DenseSide h_side{};
    h_side.cap_entries = side_size.cap_entries; h_side.cap_bytes = side_size.cap_bytes;
    SAM_TRY(hipMemcpyAsync(d_side, &h_side, sizeof h_side, hipMemcpyHostToDevice, st));
    SAM_TRY(hipMemsetAsync(pay + (size_t)units * 8, 0, 64, st));      // (a lane's 16-byte loads may overhang the last read)
    std::unique_ptr<midas_bam, void (*)(midas_bam*)> b(bam_new_columns_handle(path, names, lens), midas_bam_close);
    int32_t* h_refid = b ? bam_alloc_host_refid(b.get(), n) : nullptr;
    if (!h_refid) return sam_err(err256, MIDAS_SNPS_ERR_OUT_OF_MEMORY, "%s: out of host memory for %lld records", path, n);
    DeviceDecodeResult res;
    ResidentReads& rr = res.resident;
    rr.rec = cb + col_at[0]; rr.payload = pay;
    rr.refid = reinterpret_cast<int32_t*>(cb + col_at[1]); rr.pos = reinterpret_cast<int32_t*>(cb + col_at[2]); rr.nm = reinterpret_cast<int32_t*>(cb + col_at[3]);
    rr.l_seq = reinterpret_cast<int32_t*>(cb + col_at[4]); rr.mapq = cb + col_at[5]; rr.flag = reinterpret_cast<uint16_t*>(cb + col_at[6]);
    rr.seq_off = reinterpret_cast<int64_t*>(cb + col_at[7]); rr.qual_off = reinterpret_cast<int64_t*>(cb + col_at[8]);
    rr.cigar_off = reinterpret_cast<int64_t*>(cb + col_at[9]); rr.unit_off = reinterpret_cast<int64_t*>(cb + col_at[10]);
    rr.stream = nullptr; rr.rec_off = nullptr;       // (no text is kept: raw columns come out of the direct layout)
    rr.payload_units = (int64_t)units;
    rr.side = d_side;
    if (n > 0) {
      SamDirectP g{};
      g.perm = perm; g.n = n; g.in = cols;
      g.at_seq = sz + 6 * n1; g.at_qual = sz + 7 * n1; g.at_cigar = sz + 8 * n1; g.at_unit = sz + 9 * n1;
      g.rec = static_cast<DirectRec*>(rr.rec); g.payload = pay;
      g.refid = rr.refid; g.pos = rr.pos; g.nm = rr.nm; g.l_seq = rr.l_seq; g.mapq = rr.mapq; g.flag = rr.flag;
      g.seq_off = reinterpret_cast<long long*>(rr.seq_off); g.qual_off = reinterpret_cast<long long*>(rr.qual_off);
      g.cigar_off = reinterpret_cast<long long*>(rr.cigar_off); g.unit_off = reinterpret_cast<long long*>(rr.unit_off);
      g.side = d_side;
      const long long cap = (long long)ctx->prop.multiProcessorCount * 16;
      const long long blocks = std::max(1ll, std::min(((long long)n + 7) / 8, cap));
      hipLaunchKernelGGL(sam_direct_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g);
      SAM_TRY(hipGetLastError());
      SAM_TRY(hipMemcpyAsync(&h_side, d_side, sizeof h_side, hipMemcpyDeviceToHost, st));
      SAM_TRY(hipStreamSynchronize(st));
      g_seq.drop(); g_qual.drop(); g_cigar.drop();       // the file-order payload is gathered: it is not resident beyond this point
      lap(6);
      // (sized from pass 2's flags for exactly the reads that reserve: no room is an error of this code, not a reason to retry)
      if ((h_side.flags & kDenseSideOverflow) || (h_side.bump >> kDenseSideEntryShift) != side_size.cap_entries ||
          ((h_side.bump & kDenseSideMaxField) << 3) != side_size.cap_bytes)
        return sam_err(err256, MIDAS_SNPS_ERR_HIP, "%s: kDenseSideOverflow: the side buffer sized for %lld exceptional reads did not hold them", path,
                       (long long)side_size.cap_entries);
      SAM_TRY(hipMemcpy(h_refid, rr.refid, (size_t)n * 4, hipMemcpyDeviceToHost));
    } else {
      SAM_TRY(hipMemsetAsync(cb, 0, col_bytes, st));
      SAM_TRY(hipStreamSynchronize(st));
    }
    lap(7);
    rr.dense_flags = h_side.flags;
    res.n_records = n; res.seq_bytes = tot_seq; res.qual_bytes = tot_qual; res.n_cigar = tot_cigar;
    res.dev_owner = res_own.release();
    res.dev_free = sam_payload_free;
    bam_resident_ready(b.get(), res);
    if (n_reads) *n_reads = n;
    if (seq_bytes) *seq_bytes = tot_seq;
    if (qual_bytes) *qual_bytes = tot_qual;
    if (n_cigar) *n_cigar = tot_cigar;
    for (int k = 0; k < 8; ++k) ctx->sam_ms[k] = ms[k];
    *out = b.release();
    return MIDAS_SNPS_OK;
  }
  const size_t at_q = up((size_t)tot_seq + 64), at_c = at_q + up((size_t)tot_qual + 64), pay_bytes = at_c + up((size_t)tot_cigar * 4 + 64);
  struct Own { void* p = nullptr; ~Own() { if (p) (void)hipFree(p); } } own;
  SAM_TRY(hipMalloc(&own.p, pay_bytes));
  uint8_t* pay = static_cast<uint8_t*>(own.p);
  SAM_TRY(hipMemsetAsync(pay + tot_seq, 0, 64, st));
  SAM_TRY(hipMemsetAsync(pay + at_q + tot_qual, 0, 64, st));
  SAM_TRY(hipMemsetAsync(pay + at_c + (size_t)tot_cigar * 4, 0, 64, st));
  std::unique_ptr<midas_bam, void (*)(midas_bam*)> b(bam_new_columns_handle(path, names, lens), midas_bam_close);
  HostColumns hc{};
  if (!b || !bam_alloc_host_columns(b.get(), n, &hc)) return sam_err(err256, MIDAS_SNPS_ERR_OUT_OF_MEMORY, "%s: out of host memory for %lld records", path, n);
  if (n > 0) {
    uint32_t *vs = nullptr, *scratch = nullptr, *sz = nullptr;
    const int32_t sst = sort_records(&vs, &scratch);
    if (sst != MIDAS_SNPS_OK) return sst;
    SAM_TRY(dev.get(&sz, 6 * n1 * 4));
    uint32_t *sz_seq = sz, *sz_qual = sz + n1, *sz_cigar = sz + 2 * n1, *at_seq = sz + 3 * n1, *at_qual = sz + 4 * n1, *at_cigar = sz + 5 * n1;
    hipLaunchKernelGGL(sam_sorted_sizes_kernel, dim3(nblocks((long long)n1, 256)), dim3(256), 0, st, vs, cols.l_seq, cols.n_cigar, n, sz_seq, sz_qual, sz_cigar);
    SAM_TRY(hipGetLastError());
    SAM_TRY(launch_scan_u32(sz_seq, at_seq, (long long)n1, scratch, st));
    SAM_TRY(launch_scan_u32(sz_qual, at_qual, (long long)n1, scratch, st));
    SAM_TRY(launch_scan_u32(sz_cigar, at_cigar, (long long)n1, scratch, st));
    // the sorted small columns: one buffer, copied down column by column
    uint8_t* small = nullptr;
    const size_t o_pos = up((size_t)n * 4), o_nm = o_pos + up((size_t)n * 4), o_l = o_nm + up((size_t)n * 4), o_flag = o_l + up((size_t)n * 4),
                 o_mapq = o_flag + up((size_t)n * 2), o_so = o_mapq + up((size_t)n), o_qo = o_so + up(n1 * 8), o_co = o_qo + up(n1 * 8),
                 small_bytes = o_co + up(n1 * 8);
    SAM_TRY(dev.get(&small, small_bytes));
    SamGatherP g{};
    g.perm = vs; g.n = n; g.in = cols; g.at_seq = at_seq; g.at_qual = at_qual; g.at_cigar = at_cigar;
    g.out.refid = reinterpret_cast<int32_t*>(small); g.out.pos = reinterpret_cast<int32_t*>(small + o_pos); g.out.nm = reinterpret_cast<int32_t*>(small + o_nm);
    g.out.l_seq = reinterpret_cast<int32_t*>(small + o_l); g.out.flag = reinterpret_cast<uint16_t*>(small + o_flag); g.out.mapq = small + o_mapq;
    g.out.n_cigar = nullptr;
    g.out.seq_off = reinterpret_cast<long long*>(small + o_so); g.out.qual_off = reinterpret_cast<long long*>(small + o_qo);
    g.out.cigar_off = reinterpret_cast<long long*>(small + o_co);
    g.out.seq4 = pay; g.out.qual = pay + at_q; g.out.cigar = reinterpret_cast<uint32_t*>(pay + at_c);
    hipLaunchKernelGGL(sam_gather_kernel, dim3(nblocks((long long)n1, 4)), dim3(256), 0, st, g);
    SAM_TRY(hipGetLastError());
    SAM_TRY(hipStreamSynchronize(st));
    g_seq.drop(); g_qual.drop(); g_cigar.drop();       // the file-order payload is gathered: it is not resident beyond this point
    lap(6);
    // the small columns come down in one copy
    std::vector<uint8_t> down;
    try { down.resize(small_bytes); } catch (...) { return sam_err(err256, MIDAS_SNPS_ERR_OUT_OF_MEMORY, "%s: out of host memory for %lld records", path, n); }
    SAM_TRY(hipMemcpy(down.data(), small, small_bytes, hipMemcpyDeviceToHost));
    memcpy(hc.refid, down.data(), (size_t)n * 4); memcpy(hc.pos, down.data() + o_pos, (size_t)n * 4); memcpy(hc.nm, down.data() + o_nm, (size_t)n * 4);
    memcpy(hc.l_seq, down.data() + o_l, (size_t)n * 4); memcpy(hc.flag, down.data() + o_flag, (size_t)n * 2); memcpy(hc.mapq, down.data() + o_mapq, (size_t)n);
    memcpy(hc.seq_off, down.data() + o_so, n1 * 8); memcpy(hc.qual_off, down.data() + o_qo, n1 * 8); memcpy(hc.cigar_off, down.data() + o_co, n1 * 8);
  } else {
    hc.seq_off[0] = hc.qual_off[0] = hc.cigar_off[0] = 0;
    SAM_TRY(hipStreamSynchronize(st));
  }
  lap(7);
#undef SAM_TRY
  bam_set_device_payload(b.get(), pay, pay + at_q, pay + at_c, own.p, device_free);
  own.p = nullptr;
  bam_columns_ready(b.get(), n);
  if (n_reads) *n_reads = n;
  if (seq_bytes) *seq_bytes = tot_seq;
  if (qual_bytes) *qual_bytes = tot_qual;
  if (n_cigar) *n_cigar = tot_cigar;
  for (int k = 0; k < 8; ++k) ctx->sam_ms[k] = ms[k];
  *out = b.release();
  return MIDAS_SNPS_OK;
}

}  // namespace

extern "C" int32_t midas_sam_load_device(const char* path, midas_snps_ctx* ctx, midas_bam** out, int64_t* n_reads, int64_t* seq_bytes,
                                         int64_t* qual_bytes, int64_t* n_cigar, char* err256) {
  return sam_load(path, ctx, MIDAS_SAM_ORDER_COORDINATE, false, out, n_reads, seq_bytes, qual_bytes, n_cigar, err256);
}

extern "C" int32_t midas_sam_load_resident(const char* path, midas_snps_ctx* ctx, midas_bam** out, int64_t* n_reads, int64_t* sum_l_seq, char* err256) {
  return sam_load(path, ctx, MIDAS_SAM_ORDER_COORDINATE, true, out, n_reads, nullptr, sum_l_seq, nullptr, err256);      // (QUAL holds one byte per base)
}

extern "C" int32_t midas_sam_load_device_order(const char* path, midas_snps_ctx* ctx, int32_t order, midas_bam** out, int64_t* n_reads,
                                               int64_t* seq_bytes, int64_t* qual_bytes, int64_t* n_cigar, char* err256) {
  return sam_load(path, ctx, order, false, out, n_reads, seq_bytes, qual_bytes, n_cigar, err256);
}
