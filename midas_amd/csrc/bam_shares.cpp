// A rank's part of a BAM: slices of the file's bytes walked for their facts, contiguous shares cut at reference borders (with the
// whole block table or a rank's local one), and the record ranges a rank then loads, on the host or on the device.
#include "hostio_internal.h"

namespace {

bool plausible_record(BamWindow& w, uint64_t u, const std::vector<int64_t>& ref_lens, uint32_t* block_size) {
  if (!w.need(u, 36)) return false;
  uint64_t need = 0;
  if (plausible_bytes(w.at(u), 36, ref_lens, block_size, &need)) return true;
  if (need <= 36 || !w.need(u, need)) return false;
  return plausible_bytes(w.at(u), need, ref_lens, block_size, &need);
}

// The first offset >= from where `chain` records in a row are plausible (or the file ends exactly behind fewer).
int64_t guess_record_start(BamWindow& w, uint64_t from, const std::vector<int64_t>& ref_lens, int chain) {
  const uint64_t total = w.m->total;
  for (uint64_t u = from; u + 36 <= total; ++u) {
    uint64_t v = u;
    int ok = 0;
    while (ok < chain) {
      if (v == total) break;                       // the file ends on a record boundary: as good as a full chain
      uint32_t bs = 0;
      if (!plausible_record(w, v, ref_lens, &bs)) { ok = -1; break; }
      v += 4ull + bs;
      if (v > total) { ok = -1; break; }
      ++ok;
    }
    if (ok >= 0) return (int64_t)u;
  }
  return (int64_t)total;
}

// One record's contribution to a slice's facts (the same bookkeeping for the host's walk and the device's columns)
struct SliceFold {
  midas_bam* b;
  int32_t prev_ref = -1;
  int64_t prev_pos = -1, mark_bin = 0;
  void mapped(int32_t refid, int64_t pos, int64_t span, int64_t l_seq, uint64_t u, bool after_unmapped) {
    if (after_unmapped || refid < prev_ref) b->slice_sorted = 0;
    if (refid == prev_ref && pos < prev_pos) b->slice_pos_sorted = 0;
    if (b->slice_first_ref < 0) { b->slice_first_ref = refid; b->slice_first_pos = pos; }
    b->slice_last_ref = refid;
    b->slice_last_pos = pos;
    if (refid != prev_ref) mark_bin = 0;
    prev_ref = refid;
    prev_pos = pos;
    if (span > b->ref_span[refid]) b->ref_span[refid] = span;
    const int64_t bin = pos > 0 ? pos / MIDAS_BAM_MARK_SPAN : 0;
    if (bin > mark_bin) {
      b->marks.push_back(refid); b->marks.push_back(bin); b->marks.push_back((int64_t)u);
      mark_bin = bin;
    }
    b->ref_reads[refid] += 1;
    b->ref_bases[refid] += l_seq;
    if (b->ref_first[refid] < 0) b->ref_first[refid] = (int64_t)u;
  }
};

// A handle over a mapped BAM: the file mapped, with its whole block table or as a rank's `local` one (no block of it walked
// yet), the header read and the per-reference facts sized.
int32_t open_mapped_bam(const char* path, bool touch, bool local, std::unique_ptr<midas_bam>& b, char* err256) {
  b.reset(new (std::nothrow) midas_bam());
  if (!b) return MIDAS_SNPS_ERR_OUT_OF_MEMORY;
  b->path = path;
  b->map.reset(new BgzfMap());
  BgzfMap& m = *b->map;
  int32_t st = local ? map_file(b->path, m, err256) : bgzf_map_file(b->path, m, err256, touch);
  if (st != MIDAS_SNPS_OK) return st;
  BamWindow w;
  if (local) {   // the BAM header: the file's first blocks (a table of its own, from offset 0, as far as the header reaches)
    m.local = true;
    midas::register_file_mapping(m.base, m.size, m.fd);
    BgzfMap head;
    head.base = m.base; head.size = m.size; head.local = true; head.fd = m.fd;
    w.m = w.growable = &head;
    st = read_bam_header(w, b.get(), "%s: not a BGZF file, or corrupt deflate data", err256);
    head.base = nullptr; head.size = 0; head.fd = -1;      // (the mapping and the descriptor are m's)
  } else {
    w.m = &m;
    st = read_bam_header(w, b.get(), "%s: corrupt deflate data", err256);
  }
  if (st != MIDAS_SNPS_OK) return st;
  const size_t n_ref = b->ref_lens.size();
  b->ref_reads.assign(n_ref, 0);
  b->ref_bases.assign(n_ref, 0);
  b->ref_first.assign(n_ref, -1);
  b->ref_span.assign(n_ref, 0);
  return MIDAS_SNPS_OK;
}
}  // namespace

extern "C" int32_t midas_bam_open_slice(const char* path, int32_t slice, int32_t n_slices, midas_bam** out, char* err256) {
  return midas::bam_open_slice_with(path, slice, n_slices, nullptr, out, err256);
}

int32_t midas::bam_open_slice_with(const char* path, int32_t slice, int32_t n_slices, const midas::DeviceDecoder* dec, midas_bam** out, char* err256) {
  if (!path || !out || n_slices < 1 || slice < 0 || slice >= n_slices) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  std::unique_ptr<midas_bam> b;
  const int32_t st = open_mapped_bam(path, n_slices == 1, false, b, err256);
  if (st != MIDAS_SNPS_OK) return st;
  const BgzfMap& m = *b->map;
  const size_t nb = m.blocks.size(), rec_begin = b->rec_begin, n_ref = b->ref_lens.size();
  // this slice's blocks: those whose file offset falls into its share of the file's bytes
  const size_t b_lo = slice == 0 ? 0 : m.first_block_at((size_t)((unsigned __int128)m.size * slice / n_slices));
  const size_t b_hi = slice + 1 == n_slices ? nb : m.first_block_at((size_t)((unsigned __int128)m.size * (slice + 1) / n_slices));
  const uint64_t u_lo = std::max<uint64_t>(b_lo < nb ? m.blocks[b_lo].upos : m.total, rec_begin);
  const uint64_t u_hi = std::max<uint64_t>(b_hi < nb ? m.blocks[b_hi].upos : m.total, rec_begin);
  BamWindow w;
  w.m = &m;
  w.b_lo = w.b_hi = m.block_holding(u_lo);      // the window starts at the block holding u_lo
  if (dec && u_lo < u_hi && w.b_lo < nb) {
    // ---- the device: the slice's blocks (and a margin behind them, for the record that straddles the slice's end) inflated
    // and walked there; what comes down is refID / pos / l_seq / reference span / offset of every record that starts in the
    // slice, folded into the facts below exactly as the host's walk folds them
    const size_t j_lo = w.b_lo, j_hi = std::min(nb, std::max(b_hi, j_lo + 1) + 256);
    const uint64_t ubase = m.blocks[j_lo].upos;
    std::vector<midas::InflateJob> jobs;
    jobs.reserve(j_hi - j_lo);
    for (size_t j = j_lo; j < j_hi; ++j) {
      const BgzfMap::Blk& q = m.blocks[j];
      jobs.push_back({(uint64_t)q.cpos, q.upos - ubase, (uint32_t)q.clen, q.ulen, rd32(m.base + q.cpos + q.clen), 1u});
    }
    const uint64_t total = (j_hi < nb ? m.blocks[j_hi].upos : m.total) - ubase;
    midas::DecodeSegment seg;
    seg.job_lo = 0; seg.job_hi = jobs.size(); seg.from = u_lo - ubase; seg.exact = u_lo == rec_begin ? 1 : 0; seg.stop = u_hi - ubase;
    struct Cols { std::vector<int32_t> refid, pos, l_seq, span, nm; std::vector<uint8_t> mapq; std::vector<uint16_t> flag;
                  std::vector<int64_t> so, qo, co; std::vector<uint64_t> rec; bool ok = true; } cols;
    auto alloc = [](void* sp, int64_t n) -> midas::HostColumns {
      Cols* c = static_cast<Cols*>(sp);
      midas::HostColumns h{};
      try {
        const size_t n1 = n > 0 ? (size_t)n : 1;
        c->refid.resize(n1); c->pos.resize(n1); c->l_seq.resize(n1); c->span.resize(n1); c->nm.resize(n1); c->mapq.resize(n1);
        c->flag.resize(n1); c->so.resize((size_t)n + 1); c->qo.resize((size_t)n + 1); c->co.resize((size_t)n + 1); c->rec.resize(n1);
      } catch (...) { c->ok = false; return h; }
      h.refid = c->refid.data(); h.pos = c->pos.data(); h.nm = c->nm.data(); h.l_seq = c->l_seq.data(); h.mapq = c->mapq.data();
      h.flag = c->flag.data(); h.seq_off = c->so.data(); h.qual_off = c->qo.data(); h.cigar_off = c->co.data();
      h.span = c->span.data(); h.rec_off = c->rec.data();
      return h;
    };
    midas::DeviceDecodeResult res;
    int64_t bad_job = -1, bad_record = -1;
    const int32_t dst = dec->run(dec->user, m.base, jobs.data(), jobs.size(), total, &seg, 1, b->ref_lens.data(), (int32_t)n_ref, 0, 1, alloc, &cols,
                                 &res, &bad_job, &bad_record, err256);
    if (dst == MIDAS_SNPS_ERR_BAD_LAYOUT && bad_job >= 0) {
      set_err(err256, "%s: corrupt BGZF block at file offset %lld (deflate data or CRC-32)", path, (long long)m.blocks[j_lo + (size_t)bad_job].fpos);
      return dst;
    }
    if (dst != MIDAS_SNPS_OK && dst != MIDAS_SNPS_ERR_UNSUPPORTED && dst != MIDAS_SNPS_ERR_BAD_LAYOUT) return dst;
    if (dst == MIDAS_SNPS_OK && cols.ok && seg.first != ~0ull) {
      b->slice_first = (int64_t)(seg.first + ubase);
      b->slice_end = (int64_t)(seg.end + ubase);
      SliceFold fold{b.get()};
      for (int64_t i = 0; i < res.n_records; ++i) {
        const uint64_t u = cols.rec[(size_t)i] + ubase;
        fold.mapped(cols.refid[(size_t)i], cols.pos[(size_t)i], cols.span[(size_t)i], cols.l_seq[(size_t)i], u,
                    seg.first_unmapped != ~0ull && cols.rec[(size_t)i] > seg.first_unmapped);
      }
      *out = b.release();
      return MIDAS_SNPS_OK;
    }
    // (no boundary inside the slice, boundaries that did not settle, a record longer than the margin: the host's walk decides)
  }
  if (!w.extend(std::max(b_hi, w.b_lo + 1))) { set_err(err256, "%s: corrupt deflate data", path); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
  // The first record that starts in the slice: known exactly when the slice begins at the header's end, else guessed
  // (32 plausible records in a row) -- and verified by the caller against the end of the slice before.
  uint64_t u = u_lo == rec_begin ? rec_begin : (uint64_t)guess_record_start(w, u_lo, b->ref_lens, 32);
  b->slice_first = (int64_t)u;
  SliceFold fold{b.get()};
  bool seen_unmapped = false;
  while (u < u_hi && u < m.total) {
    uint32_t bs = 0;
    if (!plausible_record(w, u, b->ref_lens, &bs) || !w.need(u, 4ull + bs)) {
      set_err(err256, "%s: malformed alignment record at uncompressed byte %lld", path, (long long)u);
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
    const uint8_t* r = w.at(u);
    const int32_t refid = (int32_t)rd32(r + 4);
    if (refid >= 0) {
      // reference span: the lengths of the ops that consume reference (M, D, N, =, X)
      const uint32_t l_name = r[12], n_cig = rd16(r + 16);
      int64_t span = 0;
      if (36ull + l_name + 4ull * n_cig <= 4ull + bs) {
        const uint8_t* cg = r + 36 + l_name;
        for (uint32_t k = 0; k < n_cig; ++k) {
          const uint32_t v = rd32(cg + 4 * k), op = v & 15u;
          if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += v >> 4;
        }
      }
      fold.mapped(refid, (int32_t)rd32(r + 8), span, (int64_t)rd32(r + 20), u, seen_unmapped);
    } else {
      seen_unmapped = true;
    }
    u += 4ull + bs;
  }
  b->slice_end = (int64_t)u;
  *out = b.release();
  return MIDAS_SNPS_OK;
}

// Where a share begins: the first record of the first reference that BEGINS at or behind the share's first block (index `lo` of the
// handle's table; slice 0: the header's end).  -1: no reference border within max_walk.  The table may be a rank's local one (it
// grows along the chain as the walk needs blocks).
static int32_t share_first_record(midas_bam* b, int32_t slice, size_t lo, int64_t max_walk, int64_t* out_first, char* err256) {
  BgzfMap& m = *b->map;
  const uint64_t rec_begin = b->rec_begin;
  int64_t first = -1;
  if (slice == 0) {
    first = (int64_t)rec_begin;
  } else {
    const size_t nb = m.blocks.size();
    const uint64_t u_lo = std::max<uint64_t>(lo < nb ? m.blocks[lo].upos : m.total, rec_begin);
    if (u_lo >= m.total) {
      first = (int64_t)m.total;
    } else {
      BamWindow w;
      w.m = &m;
      w.growable = m.local ? &m : nullptr;
      w.b_lo = w.b_hi = m.block_holding(u_lo);
      if (!w.extend(w.b_lo + 2)) { set_err(err256, "%s: corrupt deflate data", b->path.c_str()); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
      const int64_t g = u_lo == rec_begin ? (int64_t)rec_begin : guess_record_start(w, u_lo, b->ref_lens, 32);
      if (g >= 0) {
        uint64_t u = (uint64_t)g;
        int32_t prev = 0x7fffffff;
        while (u < m.total && u - (uint64_t)g <= (uint64_t)max_walk) {
          uint32_t bs = 0;
          if (!plausible_record(w, u, b->ref_lens, &bs) || !w.need(u, 4ull + bs)) break;      // (a wrong guess runs into this: no boundary)
          const int32_t refid = (int32_t)rd32(w.at(u) + 4);
          if (prev != 0x7fffffff && refid != prev) { first = (int64_t)u; break; }
          prev = refid;
          u += 4ull + bs;
        }
        if (first < 0 && u >= m.total) first = (int64_t)m.total;        // the file's last reference runs to the end: an empty share
      }
    }
  }
  *out_first = first;
  return MIDAS_SNPS_OK;
}

// A rank's CONTIGUOUS share of a coordinate-sorted BAM, for the one-pass rank-local decode: the file is cut where slice
// `slice` of `n_slices` equal byte shares begins, moved FORWARD to the first record of the next reference (contig) -- found by
// inflating a few blocks on the host: a record start is guessed (32 plausible records in a row) and the records walked until the
// refID changes, at most max_walk uncompressed bytes.  out3 = {first, total, rec_begin}: first = uncompressed offset of the
// share's first record (the header's end for slice 0; -1: no contig border within max_walk, or no boundary could be guessed --
// the caller then plans the old way, midas_bam_open_slice; total when the share is empty).  The boundary is a GUESS until the
// rank before has decoded its own share up to exactly this offset (midas_bam_load_ranges checks that a range ends on a record
// border).  The handle takes midas_bam_load_ranges / _device like a slice's.
int32_t midas::bam_open_share(const char* path, int32_t slice, int32_t n_slices, int64_t max_walk, midas_bam** out, int64_t* out3, char* err256) {
  if (!path || !out || !out3 || n_slices < 1 || slice < 0 || slice >= n_slices || max_walk < 0) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  std::unique_ptr<midas_bam> b;
  int32_t st = open_mapped_bam(path, n_slices == 1, false, b, err256);
  if (st != MIDAS_SNPS_OK) return st;
  const BgzfMap& m = *b->map;
  out3[1] = (int64_t)m.total;
  out3[2] = (int64_t)b->rec_begin;
  int64_t first = -1;
  st = share_first_record(b.get(), slice, m.first_block_at((size_t)((unsigned __int128)m.size * slice / n_slices)), max_walk, &first, err256);
  if (st != MIDAS_SNPS_OK) return st;
  out3[0] = first;
  b->slice_first = first;
  b->slice_end = first;
  *out = b.release();
  return MIDAS_SNPS_OK;
}

extern "C" {
int32_t midas_bam_open_share(const char* path, int32_t slice, int32_t n_slices, int64_t max_walk, midas_bam** out, int64_t* out3, char* err256) {
  return midas::bam_open_share(path, slice, n_slices, max_walk, out, out3, err256);
}

// The same share with a LOCAL block table: a rank of N walks the BGZF chain over ITS 1 / N of the file's bytes only (eight ranks
// that each walk -- and page in the headers of -- the whole of a 9 GB file spend a third of a second each on it, more than on
// decoding their share).  The rank finds the first block start at or behind size * slice / n (a header from which eight headers in
// a row follow one another: a GUESS), walks the chain to the first block start at or behind size * (slice + 1) / n, and reports
//   out4 = {first block's file offset, where its walk ended, uncompressed bytes of its blocks, file size}.
// The caller exchanges these between the ranks and believes them only if they CHAIN (rank 0 starts at 0, every rank ends where the
// next one starts, the last ends at the file's end): then midas_bam_share_locate gives the table its place in the uncompressed stream
// (upos_base = the bytes of the ranks in front, total = all of them) and finds the share's first record as midas_bam_open_share does.
int32_t midas_bam_open_share_local(const char* path, int32_t slice, int32_t n_slices, midas_bam** out, int64_t* out4, char* err256) {
  if (!path || !out || !out4 || n_slices < 1 || slice < 0 || slice >= n_slices) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  std::unique_ptr<midas_bam> b;
  const int32_t st = open_mapped_bam(path, false, true, b, err256);
  if (st != MIDAS_SNPS_OK) return st;
  BgzfMap& m = *b->map;
  const size_t lo = (size_t)((unsigned __int128)m.size * slice / n_slices);
  const size_t hi = slice + 1 == n_slices ? m.size : (size_t)((unsigned __int128)m.size * (slice + 1) / n_slices);
  const size_t start = slice == 0 ? 0 : bgzf_find_block(m.base, m.size, lo, 8);
  m.next_fpos = start;
  if (!bgzf_walk_on(m, hi, ~(size_t)0)) { set_err(err256, "%s: not a BGZF block at offset %lld", path, (long long)m.next_fpos); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
  uint64_t sum = 0;
  for (const BgzfMap::Blk& q : m.blocks) sum += q.ulen;
  out4[0] = (int64_t)start; out4[1] = (int64_t)m.next_fpos; out4[2] = (int64_t)sum; out4[3] = (int64_t)m.size;
  b->slice_first = b->slice_end = -1;
  *out = b.release();
  return MIDAS_SNPS_OK;
}

int32_t midas_bam_share_locate(midas_bam* b, int32_t slice, int64_t upos_base, int64_t total, int64_t max_walk, int64_t* out3, char* err256) {
  if (!b || !b->map || !b->map->local || !out3 || upos_base < 0 || total < upos_base || max_walk < 0 || slice < 0) return MIDAS_SNPS_ERR_INVALID_ARG;
  BgzfMap& m = *b->map;
  if (m.total != 0) return MIDAS_SNPS_ERR_INVALID_ARG;       // (located once)
  for (BgzfMap::Blk& q : m.blocks) q.upos += (uint64_t)upos_base;
  if (m.blocks.empty()) {        // (an empty share: its walk goes on from where it would have begun, at the base it was given)
    // grow() continues behind the last block; with none it starts at 0 -- the first one it finds is put at the base
    if (bgzf_grow(m, 1)) m.blocks.back().upos = (uint64_t)upos_base;
  }
  m.total = (uint64_t)total;
  int64_t first = -1;
  const int32_t st = share_first_record(b, slice, 0, max_walk, &first, err256);
  if (st != MIDAS_SNPS_OK) return st;
  out3[0] = first; out3[1] = total; out3[2] = (int64_t)b->rec_begin;
  b->slice_first = b->slice_end = first;
  return MIDAS_SNPS_OK;
}
}

extern "C" {

int32_t midas_bam_slice_facts(const midas_bam* b, int64_t* out7, int64_t* ref_reads, int64_t* ref_bases, int64_t* ref_first) {
  if (!b || !b->map || !out7) return MIDAS_SNPS_ERR_INVALID_ARG;
  out7[0] = b->slice_first; out7[1] = b->slice_end; out7[2] = b->slice_sorted; out7[3] = b->slice_first_ref;
  out7[4] = b->slice_last_ref; out7[5] = (int64_t)b->rec_begin; out7[6] = (int64_t)b->map->total;
  const size_t n = b->ref_lens.size();
  if (ref_reads) memcpy(ref_reads, b->ref_reads.data(), n * 8);
  if (ref_bases) memcpy(ref_bases, b->ref_bases.data(), n * 8);
  if (ref_first) memcpy(ref_first, b->ref_first.data(), n * 8);
  return MIDAS_SNPS_OK;
}

int32_t midas_bam_slice_marks(const midas_bam* b, int64_t* out4, int64_t* ref_span, int64_t* marks, int64_t marks_capacity) {
  if (!b || !b->map || !out4) return MIDAS_SNPS_ERR_INVALID_ARG;
  const int64_t n = (int64_t)(b->marks.size() / 3);
  out4[0] = b->slice_pos_sorted; out4[1] = b->slice_first_pos; out4[2] = b->slice_last_pos; out4[3] = n;
  if (ref_span) memcpy(ref_span, b->ref_span.data(), b->ref_span.size() * 8);
  if (marks) {
    if (marks_capacity < n) return MIDAS_SNPS_ERR_INVALID_ARG;
    memcpy(marks, b->marks.data(), (size_t)n * 24);
  }
  return MIDAS_SNPS_OK;
}

int32_t midas_bam_load_ranges(midas_bam* b, int32_t n_ranges, const int64_t* range_begin, const int64_t* range_end,
                              int64_t* n_reads, int64_t* seq_bytes, int64_t* qual_bytes, int64_t* n_cigar, char* err256) {
  return midas::bam_load_ranges_with(b, nullptr, n_ranges, range_begin, range_end, n_reads, seq_bytes, qual_bytes, n_cigar, err256);
}
}  // extern "C"

// What both range loaders ask first: a handle with a map and sane arguments; a rank's local table walked on until it covers the
// ranges' far end, with no range in front of its first block; every range inside the file and behind the header.
static int32_t check_ranges(midas_bam* b, int32_t n_ranges, const int64_t* range_begin, const int64_t* range_end, char* err256) {
  if (!b || !b->map || n_ranges < 0 || (n_ranges > 0 && (!range_begin || !range_end))) return MIDAS_SNPS_ERR_INVALID_ARG;
  BgzfMap& gm = *b->map;
  if (gm.local) {
    uint64_t far = 0;
    for (int32_t k = 0; k < n_ranges; ++k) far = std::max<uint64_t>(far, (uint64_t)std::max<int64_t>(0, range_end[k]));
    while ((gm.blocks.empty() || gm.blocks.back().upos + gm.blocks.back().ulen < far) && bgzf_grow(gm, 64)) {}
    for (int32_t k = 0; k < n_ranges; ++k)
      if (range_end[k] > range_begin[k] && (gm.blocks.empty() || (uint64_t)range_begin[k] < gm.blocks[0].upos)) {
        set_err(err256, "%s: record range %lld begins in front of this rank's share of the file", b->path.c_str(), (long long)k);
        return MIDAS_SNPS_ERR_INVALID_ARG;
      }
  }
  for (int32_t k = 0; k < n_ranges; ++k)
    if (range_begin[k] < (int64_t)b->rec_begin || range_end[k] < range_begin[k] || (uint64_t)range_end[k] > gm.total) {
      set_err(err256, "%s: record range %lld outside the file", b->path.c_str(), (long long)k);
      return MIDAS_SNPS_ERR_INVALID_ARG;
    }
  return MIDAS_SNPS_OK;
}

// A rank's record ranges decoded on the device: every range is a segment of its own (the blocks from the one holding its first
// byte to the one holding its last), its first record known exactly; SEQ / QUAL / CIGAR stay on the device.
int32_t midas::bam_load_ranges_on_device(midas_bam* b, const midas::DeviceDecoder* dec, int32_t n_ranges, const int64_t* range_begin,
                                         const int64_t* range_end, int64_t* n_reads, int64_t* seq_bytes, int64_t* qual_bytes,
                                         int64_t* n_cigar, char* err256, int payload) {
  const int32_t cst = dec ? check_ranges(b, n_ranges, range_begin, range_end, err256) : MIDAS_SNPS_ERR_INVALID_ARG;
  if (cst != MIDAS_SNPS_OK) return cst;
  const BgzfMap& m = *b->map;
  std::vector<midas::InflateJob> jobs;
  std::vector<midas::DecodeSegment> segs;
  std::vector<size_t> job_block;
  uint64_t at = 0;
  for (int32_t k = 0; k < n_ranges; ++k) {
    if (range_end[k] == range_begin[k]) continue;
    const size_t b0 = m.block_holding((uint64_t)range_begin[k]), b1 = m.block_holding((uint64_t)range_end[k] - 1);
    midas::DecodeSegment sg;
    sg.job_lo = jobs.size();
    const uint64_t seg_base = at, ubase = m.blocks[b0].upos;
    for (size_t j = b0; j <= b1; ++j) {
      const BgzfMap::Blk& q = m.blocks[j];
      jobs.push_back({(uint64_t)q.cpos, at, (uint32_t)q.clen, q.ulen, rd32(m.base + q.cpos + q.clen), 1u});
      job_block.push_back(j);
      at += q.ulen;
    }
    sg.job_hi = jobs.size();
    sg.from = seg_base + ((uint64_t)range_begin[k] - ubase);
    sg.exact = 1;
    sg.stop = seg_base + ((uint64_t)range_end[k] - ubase);
    segs.push_back(sg);
  }
  ColumnSink sink{b, true, payload};
  midas::DeviceDecodeResult res;
  int64_t bad_job = -1, bad_record = -1;
  if (b->dev_free && b->dev_owner) { b->dev_free(b->dev_owner); b->dev_owner = nullptr; }      // (a handle is loaded once; be safe)
  if (segs.empty()) {
    payload = 1;        // (nothing to decode: an empty handle of the ordinary kind)
    midas::HostColumns c{};
    if (!alloc_host_columns(b, 0, &c)) { set_err(err256, "out of memory decoding %s", b->path.c_str()); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
    b->seq_off[0] = b->qual_off[0] = b->cigar_off[0] = 0;
  } else {
    const int32_t st = dec->run(dec->user, m.base, jobs.data(), jobs.size(), at, segs.data(), segs.size(), b->ref_lens.data(), (int32_t)b->ref_lens.size(),
                                payload, 0, ColumnSink::alloc, &sink, &res, &bad_job, &bad_record, err256);
    if (st == MIDAS_SNPS_ERR_BAD_LAYOUT)
      set_decode_error(err256, b->path.c_str(), bad_job >= 0 && (size_t)bad_job < job_block.size() ? (long long)m.blocks[job_block[(size_t)bad_job]].fpos : -1,
                       bad_record, "%s: record range ends inside a record");
    if (st != MIDAS_SNPS_OK) return st;
    if (!sink.ok) { if (res.dev_free && res.dev_owner) res.dev_free(res.dev_owner); set_err(err256, "out of memory decoding %s", b->path.c_str()); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
    for (const midas::DecodeSegment& sg : segs) {
      if (sg.end != sg.stop) {         // the chain from the range's first record must land exactly on its end
        if (res.dev_free && res.dev_owner) res.dev_free(res.dev_owner);
        set_err(err256, "%s: record range ends inside a record", b->path.c_str());
        return MIDAS_SNPS_ERR_BAD_LAYOUT;
      }
    }
  }
  adopt_device_result(b, res, payload);
  report_totals(res.n_records, res.seq_bytes, res.qual_bytes, res.n_cigar, n_reads, seq_bytes, qual_bytes, n_cigar);
  return MIDAS_SNPS_OK;
}

int32_t midas::bam_load_ranges_with(midas_bam* b, const midas::BlockInflater* inflater, int32_t n_ranges, const int64_t* range_begin,
                                    const int64_t* range_end, int64_t* n_reads, int64_t* seq_bytes, int64_t* qual_bytes,
                                    int64_t* n_cigar, char* err256) {
  const int32_t cst = check_ranges(b, n_ranges, range_begin, range_end, err256);
  if (cst != MIDAS_SNPS_OK) return cst;
  const BgzfMap& m = *b->map;
  const size_t nb = m.blocks.size();
  // the blocks the ranges touch, in file order, inflated back to back into one buffer
  std::vector<char> needed(nb, 0);
  for (int32_t k = 0; k < n_ranges; ++k) {
    if (range_end[k] == range_begin[k]) continue;
    for (size_t i = m.block_holding((uint64_t)range_begin[k]), e = m.block_holding((uint64_t)range_end[k] - 1); i <= e; ++i) needed[i] = 1;
  }
  std::vector<size_t> at(nb, 0), list;
  size_t bytes = 0;
  for (size_t i = 0; i < nb; ++i)
    if (needed[i]) { at[i] = bytes; bytes += m.blocks[i].ulen; list.push_back(i); }
  RawBuf<uint8_t> buf;
  if (!buf.resize(bytes)) { set_err(err256, "out of memory inflating %s", b->path.c_str()); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
  std::atomic<long long> bad{-1};
  if (inflater) {
    // runs of consecutive blocks are consecutive in the file: one segment each
    std::vector<midas::InflateSegment> segs;
    std::vector<midas::InflateJob> jobs;
    jobs.reserve(list.size());
    uint64_t cat = 0;
    for (size_t k = 0; k < list.size(); ++k) {
      const BgzfMap::Blk& blk = m.blocks[list[k]];
      const bool joins = k > 0 && list[k] == list[k - 1] + 1;
      if (!joins) {
        if (!segs.empty()) cat += segs.back().n;
        segs.push_back({m.base + blk.fpos, 0});
      }
      // (a block's stream lies between its header and its 8-byte footer; the segment runs on to the end of the block)
      const uint64_t seg_base = cat;
      jobs.push_back({seg_base + (uint64_t)(blk.cpos - (size_t)(segs.back().p - m.base)), (uint64_t)at[list[k]], (uint32_t)blk.clen, blk.ulen,
                      rd32(m.base + blk.cpos + blk.clen), 1u});
      segs.back().n = (size_t)(blk.cpos + blk.clen + 8 - (size_t)(segs.back().p - m.base));
    }
    int64_t bad_job = -1;
    const int32_t ist = inflater->run(inflater->user, segs.data(), segs.size(), jobs.data(), jobs.size(), buf.data(), bytes, &bad_job, err256);
    if (ist == MIDAS_SNPS_ERR_BAD_LAYOUT) bad = bad_job >= 0 && (size_t)bad_job < list.size() ? (long long)m.blocks[list[(size_t)bad_job]].fpos : 0;
    else if (ist != MIDAS_SNPS_OK) return ist;
  } else {
  run_pool(hw_threads(0), list.size(), [&](size_t k) {
    const BgzfMap::Blk& blk = m.blocks[list[k]];
    if (!bgzf_block_inflate(m.base + blk.cpos, (size_t)blk.clen, buf.data() + at[list[k]], (size_t)blk.ulen)) bad = (long long)blk.fpos;
  });
  }
  if (bad >= 0) { set_err(err256, "%s: corrupt BGZF block at file offset %lld (deflate data or CRC-32)", b->path.c_str(), (long long)bad.load()); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
  // walk every range from its first record to exactly its end (a range's blocks are consecutive in the buffer)
  std::vector<size_t> offs;
  for (int32_t k = 0; k < n_ranges; ++k) {
    if (range_end[k] == range_begin[k]) continue;
    const size_t b0 = m.block_holding((uint64_t)range_begin[k]);
    const size_t base = at[b0] - 0;
    const uint64_t ubase = m.blocks[b0].upos;
    uint64_t u = (uint64_t)range_begin[k];
    const uint64_t ue = (uint64_t)range_end[k];
    while (u < ue) {
      const size_t p = base + (size_t)(u - ubase);
      if (u + 36 > ue) { set_err(err256, "%s: record range ends inside a record at byte %lld", b->path.c_str(), (long long)u); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
      const uint32_t bs = rd32(&buf[p]);
      if (bs < 32 || u + 4ull + bs > ue) { set_err(err256, "%s: record range ends inside a record at byte %lld", b->path.c_str(), (long long)u); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
      if ((int32_t)rd32(&buf[p + 4]) >= 0) offs.push_back(p);
      u += 4ull + bs;
    }
  }
  const int32_t st = decode_records(b, buf.data(), offs, err256);
  if (st != MIDAS_SNPS_OK) return st;
  report_totals((int64_t)b->n_records, (int64_t)b->seq4.size(), (int64_t)b->qual.size(), (int64_t)b->cigar.size(), n_reads, seq_bytes, qual_bytes, n_cigar);
  return MIDAS_SNPS_OK;
}
