// A whole BAM on the host: the header, the record walk and decode, the handle's accessors, and the whole-file decode handed to
// the device (bam_device.hip does the device's part).
#include "hostio_internal.h"

namespace {

// NM:i (any integer width) from the aux block, or -1.
int32_t find_nm(const uint8_t* a, const uint8_t* end) {
  while (a + 3 <= end) {
    const char t0 = (char)a[0], t1 = (char)a[1], ty = (char)a[2];
    a += 3;
    size_t sz = 0;
    switch (ty) {
      case 'A': case 'c': case 'C': sz = 1; break;
      case 's': case 'S': sz = 2; break;
      case 'i': case 'I': case 'f': sz = 4; break;
      case 'Z': case 'H': { const uint8_t* z = (const uint8_t*)memchr(a, 0, (size_t)(end - a)); if (!z) return -1; sz = (size_t)(z - a) + 1; break; }
      case 'B': {
        if (a + 5 > end) return -1;
        const char st = (char)a[0];
        const size_t cnt = rd32(a + 1);
        const size_t es = (st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : 4;
        sz = 5 + cnt * es;
        break;
      }
      default: return -1;
    }
    if (a + sz > end) return -1;
    if (t0 == 'N' && t1 == 'M') {
      switch (ty) {
        case 'c': return (int8_t)a[0];
        case 'C': return a[0];
        case 's': return (int16_t)rd16(a);
        case 'S': return rd16(a);
        case 'i': return (int32_t)rd32(a);
        case 'I': { const uint32_t v = rd32(a); return v > 0x7FFFFFFFu ? 0x7FFFFFFF : (int32_t)v; }
        default: return -1;   // NM of a non-integer type: pysam would hand back a non-int; treat as absent
      }
    }
    a += sz;
  }
  return -1;
}

constexpr size_t kHeadWords = 6;     // (walk_records below fills them)
}  // namespace

// records [offs] of the inflated bytes d -> the SoA columns of b (what fetch(contig, ...) can return: refID >= 0)
int32_t decode_records(midas_bam* b, const uint8_t* d, const std::vector<size_t>& offs, char* err256, const uint32_t* heads) {
  const size_t n = offs.size();
  b->n_records = n;
  const size_t n1 = n ? n : 1;
  if (!b->refid.resize(n1) || !b->pos.resize(n1) || !b->nm.resize(n1) || !b->l_seq.resize(n1) || !b->mapq.resize(n1) ||
      !b->flag.resize(n1) || !b->seq_off.resize(n + 1) || !b->qual_off.resize(n + 1) || !b->cigar_off.resize(n + 1)) {
    set_err(err256, "out of memory decoding %s", b->path.c_str());
    return MIDAS_SNPS_ERR_OUT_OF_MEMORY;
  }
  Lap lap("bam decode");
  // sizes first, by all threads (every record header is a cache miss), then three running sums over contiguous arrays
  b->seq_off[0] = b->qual_off[0] = b->cigar_off[0] = 0;
  const bool on_device = b->payload_on_device;     // SEQ / QUAL / CIGAR are cut on the device: the small columns are all the
  {                                                // host decodes, and it does so here, on its one visit to the record
    std::atomic<size_t> nexts{0};
    std::atomic<long long> overrun{-1};
    Workers::run(hw_threads(0), [&] {
      for (;;) {
        const size_t lo = nexts.fetch_add(8192);
        if (lo >= n) return;
        const size_t hi = std::min(n, lo + 8192);
        for (size_t i = lo; i < hi; ++i) {
          const uint8_t* r = &d[offs[i] + 4];
          // (the record's fixed part: out of the walk's copy when there is one -- no cache miss per record here)
          uint32_t hw[kHeadWords];
          if (heads) memcpy(hw, heads + i * kHeadWords, sizeof hw); else memcpy(hw, &d[offs[i]], sizeof hw);
          const uint32_t bs = hw[0];
          const uint32_t l_read_name = hw[3] & 0xFFu;
          const uint32_t n_cig = hw[4] & 0xFFFFu;
          const uint32_t l = hw[5];
          if ((uint64_t)32 + l_read_name + 4ull * n_cig + (l + 1) / 2 + l > bs) {
            long long none = -1;
            overrun.compare_exchange_strong(none, (long long)i);
          }
          b->cigar_off[i + 1] = n_cig;
          b->seq_off[i + 1] = (l + 1) / 2;
          b->qual_off[i + 1] = l;
          if (on_device) {
            b->refid[i] = (int32_t)hw[1];
            b->pos[i] = (int32_t)hw[2];
            b->mapq[i] = (uint8_t)(hw[3] >> 8);
            b->flag[i] = (uint16_t)(hw[4] >> 16);
            b->l_seq[i] = (int32_t)l;
            const uint64_t body = (uint64_t)32 + l_read_name + 4ull * n_cig + (l + 1) / 2 + l;
            b->nm[i] = body <= bs ? find_nm(r + body, r + bs) : -1;
          }
        }
      }
    });
    if (overrun.load() >= 0) {
      long long first = overrun.load();      // report the lowest one, as a serial walk would
      for (size_t i = 0; i < (size_t)first; ++i) {
        const uint8_t* r = &d[offs[i] + 4];
        if ((uint64_t)32 + r[8] + 4ull * rd16(r + 12) + (rd32(r + 16) + 1) / 2 + rd32(r + 16) > rd32(&d[offs[i]])) { first = (long long)i; break; }
      }
      set_err(err256, "%s: alignment record %lld overruns its block_size", b->path.c_str(), first);
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
    for (size_t i = 0; i < n; ++i) {
      b->cigar_off[i + 1] += b->cigar_off[i];
      b->seq_off[i + 1] += b->seq_off[i];
      b->qual_off[i + 1] += b->qual_off[i];
    }
  }
  lap("record sizes + offsets");
  if (on_device) {
    b->rec_off.assign(offs.begin(), offs.end());
    b->loaded = true;
    return MIDAS_SNPS_OK;
  }
  if (!on_device && (!b->cigar.resize((size_t)b->cigar_off[n]) || !b->seq4.resize((size_t)b->seq_off[n]) || !b->qual.resize((size_t)b->qual_off[n]))) {
    set_err(err256, "out of memory decoding %s", b->path.c_str());
    return MIDAS_SNPS_ERR_OUT_OF_MEMORY;
  }
  std::atomic<size_t> next{0};
  auto work = [&] {
    for (;;) {
      const size_t lo = next.fetch_add(4096);
      if (lo >= n) return;
      const size_t hi = std::min(n, lo + 4096);
      for (size_t i = lo; i < hi; ++i) {
        const uint8_t* r = &d[offs[i] + 4];
        const uint32_t bs = rd32(&d[offs[i]]);
        b->refid[i] = (int32_t)rd32(r);
        b->pos[i] = (int32_t)rd32(r + 4);
        const uint32_t l_read_name = r[8];
        b->mapq[i] = r[9];
        const uint32_t n_cig = rd16(r + 12);
        b->flag[i] = rd16(r + 14);
        const uint32_t l = rd32(r + 16);
        b->l_seq[i] = (int32_t)l;
        const uint8_t* q = r + 32 + l_read_name;
        if (!on_device) {
          memcpy(b->cigar.data() + b->cigar_off[i], q, 4ull * n_cig);
          memcpy(b->seq4.data() + b->seq_off[i], q + 4ull * n_cig, (l + 1) / 2);
          memcpy(b->qual.data() + b->qual_off[i], q + 4ull * n_cig + (l + 1) / 2, l);
        }
        q += 4ull * n_cig + (l + 1) / 2 + l;
        b->nm[i] = find_nm(q, r + bs);
      }
    }
  };
  const int nt = hw_threads(0);
  Workers::run(nt, work);
  lap("columns");
  b->loaded = true;
  return MIDAS_SNPS_OK;
}

namespace {
// Offsets of the alignment records with refID >= 0 in an inflated BAM stream.  The records form a chain (each one's
// block_size leads to the next), a million dependent cache misses when one core walks it.  Here every thread guesses a
// record boundary inside its piece of the stream (the first offset where eight plausible records follow one another),
// walks from there to the next piece's guess, and the pieces are then stitched IN ORDER: a piece's walk counts only if
// the chain that started at the true first record ended on exactly its guess -- then the guess was a true boundary and
// the walk is the one a single core would have made.  A piece whose guess the chain does not hit is walked again from
// where the chain stands (nothing is ever taken on plausibility alone).
// heads (optional): the six leading words of every kept record -- block_size, refID, pos, l_read_name | mapq << 8 | bin << 16,
// n_cigar_op | flag << 16, l_seq -- taken while the walk has the record's first cache line in hand anyway, so that the decoder's
// size pass (and, with the payload on the device, its whole small-column pass) never has to come back for them.
int32_t walk_records(const uint8_t* d, size_t total, size_t rec_begin, const std::vector<int64_t>& ref_lens,
                     std::vector<size_t>& offs, const char* path, char* err256, std::vector<uint32_t>* heads = nullptr) {
  struct Piece { size_t start = 0, end = 0, bad_at = 0; bool bad = false; std::vector<size_t> offs; std::vector<uint32_t> heads; };
  const bool want_heads = heads != nullptr;
  auto walk = [&](size_t p, size_t stop, Piece& pc) {     // records starting in [p, stop); pc.end = first start >= stop
    while (p + 4 <= total && p < stop) {
      const size_t bs = rd32(&d[p]);
      if (bs < 32 || p + 4 + bs > total) { pc.bad = true; pc.bad_at = p; break; }
      const int32_t rid = (int32_t)rd32(&d[p + 4]);
      if (rid >= (int32_t)ref_lens.size()) { pc.bad = true; pc.bad_at = p; break; }      // (names no reference of the header)
      if (rid >= 0) {
        pc.offs.push_back(p);
        if (want_heads) {
          uint32_t w[kHeadWords];
          memcpy(w, &d[p], sizeof w);       // (bs >= 32: the 24 bytes are the record's)
          pc.heads.insert(pc.heads.end(), w, w + kHeadWords);
        }
      }
      p += 4 + bs;
    }
    pc.end = p;
  };
  const int nt = hw_threads(0);
  const size_t span = total > rec_begin ? total - rec_begin : 0;
  size_t n_pieces = std::min<size_t>((size_t)nt * 4, span / ((size_t)1 << 20));
  if (n_pieces < 2) {
    Piece all;
    walk(rec_begin, total, all);
    if (all.bad) { set_err(err256, "%s: truncated or malformed alignment record at byte %lld", path, (long long)all.bad_at); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
    offs.swap(all.offs);
    if (want_heads) heads->swap(all.heads);
    return MIDAS_SNPS_OK;
  }
  const size_t per = span / n_pieces;
  std::vector<size_t> guess(n_pieces);
  std::atomic<size_t> next{0};
  Workers::run(nt, [&] {
    for (;;) {
      const size_t k = next.fetch_add(1);
      if (k >= n_pieces) return;
      if (k == 0) { guess[0] = rec_begin; continue; }
      size_t u = rec_begin + k * per;
      const size_t limit = std::min(total, u + per);      // a piece without a boundary of its own joins the one before
      size_t found = total;
      for (; u < limit; ++u) {
        size_t v = u;
        int ok = 0;
        while (ok < 8 && v != total) {
          uint32_t bs = 0;
          uint64_t need = 0;
          if (!plausible_bytes(d + v, total - v, ref_lens, &bs, &need) || v + 4ull + bs > total) { ok = -1; break; }
          v += 4ull + bs;
          ++ok;
        }
        if (ok >= 0) { found = u; break; }
      }
      guess[k] = found;
    }
  });
  std::vector<Piece> pieces;
  for (size_t k = 0; k < n_pieces; ++k)
    if (guess[k] < total && (pieces.empty() || guess[k] > pieces.back().start)) { pieces.emplace_back(); pieces.back().start = guess[k]; }
  next = 0;
  Workers::run(nt, [&] {
    for (;;) {
      const size_t k = next.fetch_add(1);
      if (k >= pieces.size()) return;
      pieces[k].offs.reserve(per / 200);
      if (want_heads) pieces[k].heads.reserve(per / 200 * kHeadWords);
      walk(pieces[k].start, k + 1 < pieces.size() ? pieces[k + 1].start : total, pieces[k]);
    }
  });
  size_t cur = rec_begin, n_total = 0;
  std::vector<Piece> redo(pieces.size());
  std::vector<const Piece*> use(pieces.size(), nullptr);
  for (size_t k = 0; k < pieces.size(); ++k) {
    const Piece* pc = &pieces[k];
    if (cur != pc->start) {                 // the chain did not arrive on this piece's guess: walk it from the chain's position
      const size_t stop = k + 1 < pieces.size() ? pieces[k + 1].start : total;
      if (cur < stop) walk(cur, stop, redo[k]); else redo[k].end = cur;
      pc = &redo[k];
#ifdef MIDAS_HOSTIO_TRACE
      fprintf(stderr, "[bam load] piece %zu of %zu walked again: guess %zu, chain at %zu\n", k, pieces.size(), pieces[k].start, cur);
#endif
    }
    if (pc->bad) { set_err(err256, "%s: truncated or malformed alignment record at byte %lld", path, (long long)pc->bad_at); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
    use[k] = pc;
    n_total += pc->offs.size();
    cur = pc->end;
  }
  offs.resize(n_total);
  if (want_heads) heads->resize(n_total * kHeadWords);
  std::vector<size_t> at(pieces.size() + 1, 0);
  for (size_t k = 0; k < pieces.size(); ++k) at[k + 1] = at[k] + use[k]->offs.size();
  next = 0;
  Workers::run(nt, [&] {
    for (;;) {
      const size_t k = next.fetch_add(1);
      if (k >= pieces.size()) return;
      if (!use[k]->offs.empty()) memcpy(offs.data() + at[k], use[k]->offs.data(), use[k]->offs.size() * sizeof(size_t));
      if (want_heads && !use[k]->heads.empty())
        memcpy(heads->data() + at[k] * kHeadWords, use[k]->heads.data(), use[k]->heads.size() * sizeof(uint32_t));
    }
  });
  return MIDAS_SNPS_OK;
}

}  // namespace

// What the parser says about ALL the bytes there are, as a status and a message: a header that wants more is cut off, and a
// reference table that is malformed reads the same.
static int32_t header_status(midas::BamHeader r, const char* path, char* err256) {
  if (r == midas::BamHeader::parsed) return MIDAS_SNPS_OK;
  set_err(err256, r == midas::BamHeader::bad_magic ? "%s: missing BAM magic" : "%s: truncated BAM header", path);
  return MIDAS_SNPS_ERR_BAD_LAYOUT;
}
// The BAM header out of the first blocks of the window's table into b (ref_names, ref_lens, rec_begin): as many blocks as it takes,
// twice as many every round.  corrupt_fmt: the caller's text for a block that does not inflate (path, the block's file offset).
int32_t read_bam_header(BamWindow& w, midas_bam* b, const char* corrupt_fmt, char* err256) {
  for (size_t k = 1;; k *= 2) {
    if (!w.extend(k) || (w.growable && w.b_hi == 0)) { set_err(err256, corrupt_fmt, b->path.c_str(), w.bad_fpos); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
    const midas::BamHeader r = midas::parse_bam_header(w.buf.data(), w.buf.size(), &b->ref_names, &b->ref_lens, &b->rec_begin);
    if (r != midas::BamHeader::more || w.b_hi < k) return header_status(r, b->path.c_str(), err256);      // (fewer blocks than asked for: the file has no more)
  }
}

extern "C" {

int32_t midas_bam_open(const char* path, midas_bam** out, char* err256) { return midas::bam_open_with(path, nullptr, out, err256); }
}  // extern "C"

void midas::bam_keep_payload_on_device(midas_bam* b) { b->payload_on_device = true; }
const uint64_t* midas::bam_record_offsets(const midas_bam* b, size_t* n) { *n = b->rec_off.size(); return b->rec_off.data(); }
void midas::bam_offsets(const midas_bam* b, const int64_t** seq_off, const int64_t** qual_off, const int64_t** cigar_off) {
  *seq_off = b->seq_off.data(); *qual_off = b->qual_off.data(); *cigar_off = b->cigar_off.data();
}
void midas::bam_set_device_payload(midas_bam* b, void* seq4, void* qual, void* cigar, void* owner, void (*free_fn)(void*)) {
  b->dev_payload[0] = seq4; b->dev_payload[1] = qual; b->dev_payload[2] = cigar;
  b->dev_owner = owner;
  b->dev_free = free_fn;
  std::vector<uint64_t>().swap(b->rec_off);
}

midas_bam* midas::bam_new_columns_handle(const char* path, const std::vector<std::string>& ref_names, const std::vector<int64_t>& ref_lens) {
  midas_bam* b = new (std::nothrow) midas_bam();
  if (!b) return nullptr;
  b->path = path;
  b->ref_names = ref_names;
  b->ref_lens = ref_lens;
  return b;
}
void midas::bam_columns_ready(midas_bam* b, int64_t n_records) {
  b->n_records = (size_t)n_records;
  b->loaded = true;
  b->payload_on_device = true;
}

// (a resident handle's refID column is in use -- the host holds views of it: it stays where it is)
bool midas::bam_alloc_host_columns(midas_bam* b, int64_t n, midas::HostColumns* c) { return alloc_host_columns(b, n, c, b->resident); }
const midas::ResidentReads* midas::bam_resident(const midas_bam* b, int64_t* n_records, int64_t* seq_bytes, int64_t* qual_bytes, int64_t* n_cigar) {
  if (!b || !b->resident) return nullptr;
  if (n_records) *n_records = (int64_t)b->n_records;
  if (seq_bytes) *seq_bytes = b->rr_seq_bytes;
  if (qual_bytes) *qual_bytes = b->rr_qual_bytes;
  if (n_cigar) *n_cigar = b->rr_n_cigar;
  return &b->rr;
}
void midas::bam_resident_became_columns(midas_bam* b, void* seq4, void* qual, void* cigar, void* owner, void (*free_fn)(void*)) {
  b->dev_payload[0] = seq4; b->dev_payload[1] = qual; b->dev_payload[2] = cigar;
  b->dev_owner2 = owner;
  b->dev_free2 = free_fn;
  b->payload_on_device = true;
}
// (resident decode: refID is the one column the host asks for)
static bool alloc_host_refid(midas_bam* b, int64_t n, midas::HostColumns* c) {
  if (!b->refid.resize(n > 0 ? (size_t)n : 1)) return false;
  *c = midas::HostColumns{};
  c->refid = b->refid.data();
  return true;
}
// what a device decode left in `res`, taken into the handle
void adopt_device_result(midas_bam* b, const midas::DeviceDecodeResult& res, int payload) {
  b->n_records = (size_t)res.n_records;
  b->loaded = true;
  b->dev_owner = res.dev_owner;
  b->dev_free = res.dev_free;
  if (payload == 2) {
    b->resident = true;
    b->payload_on_device = false;
    b->rr = res.resident;
    b->rr_seq_bytes = res.seq_bytes; b->rr_qual_bytes = res.qual_bytes; b->rr_n_cigar = res.n_cigar;
  } else {
    b->payload_on_device = true;
    b->dev_payload[0] = res.dev_seq; b->dev_payload[1] = res.dev_qual; b->dev_payload[2] = res.dev_cigar;
  }
}
int32_t* midas::bam_alloc_host_refid(midas_bam* b, int64_t n_records) {
  midas::HostColumns c{};
  return alloc_host_refid(b, n_records, &c) ? c.refid : nullptr;
}
void midas::bam_resident_ready(midas_bam* b, const midas::DeviceDecodeResult& res) { adopt_device_result(b, res, 2); }
bool alloc_host_columns(midas_bam* b, int64_t n, midas::HostColumns* c, bool keep_refid) {
  const size_t n1 = n > 0 ? (size_t)n : 1;
  if ((!keep_refid && !b->refid.resize(n1)) || !b->pos.resize(n1) || !b->nm.resize(n1) || !b->l_seq.resize(n1) || !b->mapq.resize(n1) ||
      !b->flag.resize(n1) || !b->seq_off.resize((size_t)n + 1) || !b->qual_off.resize((size_t)n + 1) || !b->cigar_off.resize((size_t)n + 1))
    return false;
  c->refid = b->refid.data(); c->pos = b->pos.data(); c->nm = b->nm.data(); c->l_seq = b->l_seq.data(); c->mapq = b->mapq.data();
  c->flag = b->flag.data(); c->seq_off = b->seq_off.data(); c->qual_off = b->qual_off.data(); c->cigar_off = b->cigar_off.data();
  c->span = nullptr; c->rec_off = nullptr;
  return true;
}

midas::HostColumns ColumnSink::alloc(void* sink, int64_t n) {
  ColumnSink* s = static_cast<ColumnSink*>(sink);
  midas::HostColumns c{};
  if (!(s->payload == 2 ? alloc_host_refid(s->b, n, &c) : alloc_host_columns(s->b, n, &c))) s->ok = false;
  return c;
}
// What a device decode's MIDAS_SNPS_ERR_BAD_LAYOUT was about: the block at file offset bad_fpos (-1: none is named), else record
// bad_record (< 0: none), else `otherwise` (nullptr: the decoder's own text stays).
void set_decode_error(char* err256, const char* path, long long bad_fpos, int64_t bad_record, const char* otherwise) {
  if (bad_fpos >= 0) set_err(err256, "%s: corrupt BGZF block at file offset %lld (deflate data or CRC-32)", path, bad_fpos);
  else if (bad_record >= 0) set_err(err256, "%s: alignment record %lld overruns its block_size or names no reference of the header", path, (long long)bad_record);
  else if (otherwise) set_err(err256, otherwise, path);
}

// What the whole-file device decodes share (bam_decode_on_device, bam_genes_on_device): the job table of the file's blocks, ONE
// segment from the header's end to the file's, dec->run, and its MIDAS_SNPS_ERR_BAD_LAYOUT turned into the file's text.
static int32_t decode_whole_file(const midas_bam* b, const uint8_t* base, const std::vector<FileBlk>& blocks, size_t total, const midas::DeviceDecoder* dec,
                                 int payload, midas::HostColumns (*alloc)(void*, int64_t), void* sink, midas::DeviceDecodeResult* res, char* err256) {
  std::vector<midas::InflateJob> jobs;
  jobs.reserve(blocks.size());
  for (const FileBlk& q : blocks) jobs.push_back({(uint64_t)q.cpos, (uint64_t)q.upos, (uint32_t)q.clen, (uint32_t)q.ulen, rd32(base + q.cpos + q.clen), 1u});
  int64_t bad_job = -1, bad_record = -1;
  midas::DecodeSegment seg;
  seg.job_lo = 0; seg.job_hi = jobs.size(); seg.from = (uint64_t)b->rec_begin; seg.exact = 1; seg.stop = (uint64_t)total;
  const int32_t st = dec->run(dec->user, base, jobs.data(), jobs.size(), (uint64_t)total, &seg, 1, b->ref_lens.data(), (int32_t)b->ref_lens.size(),
                              payload, 0, alloc, sink, res, &bad_job, &bad_record, err256);
  if (st == MIDAS_SNPS_ERR_BAD_LAYOUT)
    set_decode_error(err256, b->path.c_str(), bad_job >= 0 && (size_t)bad_job < blocks.size() ? (long long)blocks[(size_t)bad_job].fpos : -1, bad_record,
                     bad_record == -2 ? "%s: malformed alignment record (a block_size that leaves the stream)" : nullptr);
  return st;
}

int32_t midas::bam_decode_on_device(const char* path, const midas::DeviceDecoder* dec, midas_bam** out, int64_t* n_reads,
                                    int64_t* seq_bytes, int64_t* qual_bytes, int64_t* n_cigar, char* err256, int payload) {
  if (!path || !out || !dec) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  std::unique_ptr<midas_bam> b(new (std::nothrow) midas_bam());
  if (!b) return MIDAS_SNPS_ERR_OUT_OF_MEMORY;
  b->path = path;
  FileImage comp;
  std::vector<FileBlk> blocks;
  size_t total = 0;
  int32_t st = read_bgzf_file(b->path, comp, blocks, &total, err256);
  if (st != MIDAS_SNPS_OK) return st;
  Lap lap("bam device decode");
  {   // the header: the file's blocks lent to a table for the window that reads it
    BgzfMap view;
    view.base = comp.data(); view.size = comp.size(); view.total = total;
    view.blocks.swap(blocks);
    BamWindow w;
    w.m = &view;
    st = read_bam_header(w, b.get(), "%s: corrupt BGZF block at file offset %lld (deflate data or CRC-32)", err256);
    view.blocks.swap(blocks);
    view.base = nullptr; view.size = 0;      // (the bytes are comp's)
    if (st != MIDAS_SNPS_OK) return st;
  }
  lap("header");
  ColumnSink sink{b.get(), true, payload};
  midas::DeviceDecodeResult res;
  st = decode_whole_file(b.get(), comp.data(), blocks, total, dec, payload, ColumnSink::alloc, &sink, &res, err256);
  lap("device");
  if (st != MIDAS_SNPS_OK) return st;
  if (!sink.ok) { set_err(err256, "out of memory decoding %s", path); if (res.dev_free && res.dev_owner) res.dev_free(res.dev_owner); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
  adopt_device_result(b.get(), res, payload);
  report_totals(res.n_records, res.seq_bytes, res.qual_bytes, res.n_cigar, n_reads, seq_bytes, qual_bytes, n_cigar);
  *out = b.release();
  return MIDAS_SNPS_OK;
}

// midas_genes_count_bam (bam_device.hip): the whole file to `dec` with payload 3 (decode_whole_file) -- the
// handle's own mapping and block table when it has them (midas_bam_open_share), else the file read as bam_decode_on_device reads it.
// Nothing is loaded into the handle.
int32_t midas::bam_genes_on_device(const midas_bam* b, const midas::DeviceDecoder* dec, void* call, char* err256) {
  if (!b || !dec || !call || b->loaded) return MIDAS_SNPS_ERR_INVALID_ARG;
  FileImage comp;
  std::vector<FileBlk> own;
  const uint8_t* base = nullptr;
  const std::vector<FileBlk>* blocks = &own;
  size_t total = 0;
  if (b->map && !b->map->local) {
    base = b->map->base; blocks = &b->map->blocks; total = (size_t)b->map->total;
  } else {
    const int32_t st = read_bgzf_file(b->path, comp, own, &total, err256);
    if (st != MIDAS_SNPS_OK) return st;
    base = comp.data();
  }
  if (blocks->empty() || b->rec_begin > total) { set_err(err256, "%s: truncated BAM header", b->path.c_str()); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
  midas::DeviceDecodeResult res;
  return decode_whole_file(b, base, *blocks, total, dec, 3, nullptr, call, &res, err256);
}

int32_t midas::bam_open_with(const char* path, const midas::BlockInflater* inflater, midas_bam** out, char* err256) {
  if (!path || !out) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  std::unique_ptr<midas_bam> b(new (std::nothrow) midas_bam());
  if (!b) return MIDAS_SNPS_ERR_OUT_OF_MEMORY;
  b->path = path;
  int32_t st = bgzf_inflate_file(b->path, b->data, err256, inflater);
  if (st != MIDAS_SNPS_OK) return st;
  const RawBuf<uint8_t>& d = b->data;      // (the whole stream: fewer than the 12 bytes every header has are no BAM at all)
  st = header_status(d.size() < 12 ? midas::BamHeader::bad_magic : midas::parse_bam_header(d.data(), d.size(), &b->ref_names, &b->ref_lens, &b->rec_begin),
                     path, err256);
  if (st != MIDAS_SNPS_OK) return st;
  *out = b.release();
  return MIDAS_SNPS_OK;
}

extern "C" {

void midas_bam_close(midas_bam* b) { delete b; }

int32_t midas_bam_n_refs(const midas_bam* b) { return b ? (int32_t)b->ref_names.size() : 0; }

int32_t midas_bam_ref(const midas_bam* b, int32_t i, const char** name, int64_t* length) {
  if (!b || i < 0 || i >= (int32_t)b->ref_names.size()) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (name) *name = b->ref_names[i].c_str();
  if (length) *length = b->ref_lens[i];
  return MIDAS_SNPS_OK;
}

int32_t midas_bam_load(midas_bam* b, int64_t* n_reads, int64_t* seq_bytes, int64_t* qual_bytes, int64_t* n_cigar,
                       char* err256) {
  if (!b) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (!b->loaded) {
    const RawBuf<uint8_t>& d = b->data;
    // pass 1: record offsets (what fetch(contig, ...) can ever return: refID >= 0)
    Lap lap("bam load");
    std::vector<size_t> offs;
    std::vector<uint32_t> heads;
    const int32_t wst = walk_records(d.data(), d.size(), b->rec_begin, b->ref_lens, offs, b->path.c_str(), err256, &heads);
    if (wst != MIDAS_SNPS_OK) return wst;
    lap("record walk");
    const int32_t st = decode_records(b, d.data(), offs, err256, heads.data());
    if (st != MIDAS_SNPS_OK) return st;
    lap("decode_records");
    // the inflated stream is no longer needed; unmapping hundreds of MB takes ~10 ms, which nobody has to wait for
    std::thread([](RawBuf<uint8_t> gone) { gone.release(); }, std::move(b->data)).detach();
    lap("release");
  }
  const size_t nr = b->n_records;
  const bool dev = b->payload_on_device;
  report_totals((int64_t)nr, dev ? b->seq_off[nr] : (int64_t)b->seq4.size(), dev ? b->qual_off[nr] : (int64_t)b->qual.size(),
                dev ? b->cigar_off[nr] : (int64_t)b->cigar.size(), n_reads, seq_bytes, qual_bytes, n_cigar);
  return MIDAS_SNPS_OK;
}

int32_t midas_bam_payload_on_device(const midas_bam* b) { return b && b->payload_on_device ? 1 : 0; }

// The file's mapping is not needed any more (its records are decoded): it is taken from the handle and unmapped on a thread of
// its own.  Unmapping a BAM of gigabytes is a page-table walk of a tenth of a second and more -- time the caller can spend on
// the pileup instead of at the handle's close.  The handle keeps its columns / resident records; it cannot load ranges again.
void midas_bam_release_file(midas_bam* b) {
  if (!b || !b->map) return;
  std::thread([](std::unique_ptr<BgzfMap> gone) { gone.reset(); }, std::move(b->map)).detach();
}

int32_t midas_bam_columns(const midas_bam* b, const void** out12) {
  if (!b || !b->loaded || !out12) return MIDAS_SNPS_ERR_INVALID_ARG;
  const void* v[12] = {b->refid.data(), b->pos.data(), b->mapq.data(), b->flag.data(), b->nm.data(), b->l_seq.data(),
                       b->seq_off.data(), b->qual_off.data(), b->cigar_off.data(), b->seq4.data(), b->qual.data(),
                       b->cigar.data()};
  if (b->payload_on_device) { v[9] = b->dev_payload[0]; v[10] = b->dev_payload[1]; v[11] = b->dev_payload[2]; }
  if (b->resident && !b->payload_on_device)       // (every column but refID is on the device: midas_bam_resident_to_columns brings them)
    for (int k = 1; k < 12; ++k) v[k] = nullptr;
  memcpy(out12, v, sizeof v);
  return MIDAS_SNPS_OK;
}

int32_t midas_bam_copy(const midas_bam* b, int32_t* refid, int32_t* pos, uint8_t* mapq, uint16_t* flag, int32_t* nm,
                       int32_t* l_seq, int64_t* seq_off, int64_t* qual_off, int64_t* cigar_off, uint8_t* seq4,
                       uint8_t* qual, uint32_t* cigar) {
  if (!b || !b->loaded) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (b->payload_on_device && (seq4 || qual || cigar)) return MIDAS_SNPS_ERR_INVALID_ARG;     // (they are not in host memory)
  const size_t n = b->n_records;
  // the three big columns are copied by all cores (a single memcpy of ~250 MB is 60 ms of the stage)
  auto cp = [](void* dst, const void* src, size_t bytes) {
    if (!dst || !bytes) return;
    const size_t piece = (size_t)4 << 20;
    if (bytes < 4 * piece) { memcpy(dst, src, bytes); return; }
    const size_t n_pieces = (bytes + piece - 1) / piece;
    run_pool(hw_threads(0), n_pieces, [&](size_t i) {
      const size_t lo = i * piece, len = std::min(piece, bytes - lo);
      memcpy(static_cast<uint8_t*>(dst) + lo, static_cast<const uint8_t*>(src) + lo, len);
    });
  };
  cp(refid, b->refid.data(), n * 4); cp(pos, b->pos.data(), n * 4); cp(mapq, b->mapq.data(), n);
  cp(flag, b->flag.data(), n * 2); cp(nm, b->nm.data(), n * 4); cp(l_seq, b->l_seq.data(), n * 4);
  cp(seq_off, b->seq_off.data(), (n + 1) * 8); cp(qual_off, b->qual_off.data(), (n + 1) * 8);
  cp(cigar_off, b->cigar_off.data(), (n + 1) * 8);
  cp(seq4, b->seq4.data(), b->seq4.size()); cp(qual, b->qual.data(), b->qual.size());
  cp(cigar, b->cigar.data(), b->cigar.size() * 4);
  return MIDAS_SNPS_OK;
}
}  // extern "C"
