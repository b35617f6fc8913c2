// The pure pieces of the host's BAM reader: the header parser, the record-start plausibility check and the two searches over a
// BGZF block table.  Nothing of the library is included, so that a stand-alone program can hold them to a plain restatement
// (tests/cpp/bam_header_check.cpp).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace midas {

enum class BamHeader { parsed, more, bad_magic, bad_refs };

// The BAM header (magic, text, reference table) out of the first n inflated bytes; never reads at or beyond d + n.
//   parsed: names / lens / rec_begin (the offset of the first alignment record) are set;   more: the header runs on behind d + n;
//   bad_magic: not a BAM;   bad_refs: a reference with l_name == 0 (its name has not even the closing NUL).
static inline BamHeader parse_bam_header(const uint8_t* d, size_t n, std::vector<std::string>* names, std::vector<int64_t>* lens, size_t* rec_begin) {
  auto u32 = [&](size_t at) { uint32_t v; memcpy(&v, d + at, 4); return v; };
  if (n < 12) return BamHeader::more;      // (magic, l_text, n_ref: no header is shorter)
  if (memcmp(d, "BAM\1", 4) != 0) return BamHeader::bad_magic;
  size_t p = 8 + (size_t)u32(4);
  if (p + 4 > n) return BamHeader::more;
  const uint32_t n_ref = u32(p);
  p += 4;
  names->clear();
  lens->clear();
  for (uint32_t i = 0; i < n_ref; ++i) {
    if (p + 4 > n) return BamHeader::more;
    const uint32_t l_name = u32(p);
    p += 4;
    if (l_name == 0) return BamHeader::bad_refs;
    if (p + l_name + 4 > n) return BamHeader::more;
    names->emplace_back(reinterpret_cast<const char*>(d + p), l_name - 1);
    p += l_name;
    lens->push_back(u32(p));
    p += 4;
  }
  *rec_begin = p;
  return BamHeader::parsed;
}

// Could an alignment record start at uncompressed offset u?  Every fixed field must be plausible and the variable parts
// must fit the record's own block_size.  (A guess that passes here is only ever TRUSTED after the walk of the slice before
// it has ended on exactly this offset: midas_amd/run/snps.py checks that across ranks.)
// (r: the bytes from the candidate offset on, avail of them readable; *need: how many the full check wants, when
// more than avail are needed the answer is "false" with *need set so that the caller can map more and ask again)
static inline bool plausible_bytes(const uint8_t* r, uint64_t avail, const std::vector<int64_t>& ref_lens, uint32_t* block_size, uint64_t* need) {
  auto rd32 = [](const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; };
  auto rd16 = [](const uint8_t* p) { uint16_t v; memcpy(&v, p, 2); return v; };
  *need = 36;
  if (avail < 36) return false;
  const uint32_t bs = rd32(r);
  if (bs < 32 || bs > (1u << 26)) { *need = 0; return false; }
  const int32_t refid = (int32_t)rd32(r + 4), pos = (int32_t)rd32(r + 8);
  const uint32_t lrn = r[12], n_cig = rd16(r + 16), l = rd32(r + 20);
  const int32_t nref = (int32_t)rd32(r + 24), npos = (int32_t)rd32(r + 28);
  const int32_t n_ref = (int32_t)ref_lens.size();
  *need = 0;
  if (refid < -1 || refid >= n_ref || nref < -1 || nref >= n_ref || pos < -1 || npos < -1) return false;
  if (refid >= 0 && pos > ref_lens[refid]) return false;
  if (lrn < 1 || l > (1u << 26)) return false;
  if ((uint64_t)32 + lrn + 4ull * n_cig + (l + 1) / 2 + l > bs) return false;
  *need = 4ull + 32 + lrn + 4ull * n_cig;
  if (avail < *need) return false;
  *need = 0;
  const uint8_t* name = r + 36;
  if (name[lrn - 1] != 0) return false;
  for (uint32_t k = 0; k + 1 < lrn; ++k)
    if (name[k] < 33 || name[k] > 126) return false;
  const uint8_t* cg = name + lrn;
  for (uint32_t k = 0; k < n_cig && k < 64; ++k)
    if ((rd32(cg + 4 * k) & 15u) > 8u) return false;
  *block_size = bs;
  return true;
}

// A block table is an array of {upos, ulen, fpos, ...}: where each block's bytes lie in the inflated stream and in the file, both
// ascending.  The block holding uncompressed offset u -- the first that ends behind u; an empty block (the EOF block) holds
// nothing; nb when u is at or behind the table's end.
template <class Blk>
static inline size_t block_holding(const Blk* blocks, size_t nb, uint64_t u) {
  size_t lo = 0, hi = nb;
  while (lo < hi) { const size_t mid = (lo + hi) / 2; if (blocks[mid].upos + blocks[mid].ulen <= u) lo = mid + 1; else hi = mid; }
  return lo;
}
// The first block at or behind file offset fpos (nb: none).
template <class Blk>
static inline size_t first_block_at(const Blk* blocks, size_t nb, size_t fpos) {
  size_t lo = 0, hi = nb;
  while (lo < hi) { const size_t mid = (lo + hi) / 2; if (blocks[mid].fpos < fpos) lo = mid + 1; else hi = mid; }
  return lo;
}

}  // namespace midas
