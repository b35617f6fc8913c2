// BGZF on the host: the registry of mapped files, the inflater, a file's block table (walked with pread, by several threads), a
// file read or mapped whole, and the mapping of a BAM with its table.
#include "hostio_internal.h"

namespace {
struct MappedFile { const uint8_t* base; size_t size; int fd; };
std::mutex g_map_lock;
std::vector<MappedFile> g_maps;
}  // namespace
void midas::register_file_mapping(const void* base, size_t size, int fd) {
  std::lock_guard<std::mutex> g(g_map_lock);
  g_maps.push_back({static_cast<const uint8_t*>(base), size, fd});
}
void midas::unregister_file_mapping(const void* base) {
  std::lock_guard<std::mutex> g(g_map_lock);
  for (size_t k = 0; k < g_maps.size(); ++k)
    if (g_maps[k].base == base) { g_maps.erase(g_maps.begin() + (long)k); return; }
}
bool midas::file_of_mapping(const void* p, size_t n, int* fd, size_t* file_off) {
  const uint8_t* q = static_cast<const uint8_t*>(p);
  std::lock_guard<std::mutex> g(g_map_lock);
  for (const MappedFile& m : g_maps)
    if (q >= m.base && n <= m.size && (size_t)(q - m.base) <= m.size - n) { *fd = m.fd; *file_off = (size_t)(q - m.base); return true; }
  return false;
}


const Libdeflate& libdeflate() {
  static const Libdeflate l;
  return l;
}
namespace {
struct ThreadInflater {      // one decompressor per thread, for the thread's life
  void* d = nullptr;
  ~ThreadInflater() { if (d) libdeflate().release(d); }
};
}  // namespace
bool raw_inflate(const uint8_t* in, size_t n_in, uint8_t* out, size_t n_out) {
  const Libdeflate& l = libdeflate();
  if (l.run) {
    static thread_local ThreadInflater t;
    if (!t.d) t.d = l.alloc();
    if (t.d) {
      size_t got = 0;
      return l.run(t.d, in, n_in, out, n_out, &got) == 0 && got == n_out;
    }
  }
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, -15) != Z_OK) return false;
  zs.next_in = const_cast<Bytef*>(in);
  zs.avail_in = (uInt)n_in;
  zs.next_out = out;
  zs.avail_out = (uInt)n_out;
  const int rc = inflate(&zs, Z_FINISH);
  inflateEnd(&zs);
  return rc == Z_STREAM_END && zs.avail_out == 0;
}

// Inflate every BGZF block of a file into one buffer.  Blocks are independent raw-deflate members, so they
// are inflated in parallel once the block boundaries are known (BSIZE in the 'BC' extra field).
// A BGZF block header in h[0, avail) (an extra field with the BC subfield, as htslib and this library write it): its XLEN and BSIZE.
static bool bgzf_parse_header(const uint8_t* h, size_t avail, size_t* xlen_out, size_t* bsize_out) {
  if (avail < 18 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return false;
  const size_t xlen = rd16(&h[10]);
  if (12 + xlen > avail) return false;
  size_t q = 12, xend = 12 + xlen, bsize = 0;
  while (q + 4 <= xend) {
    const uint16_t slen = rd16(&h[q + 2]);
    if (h[q] == 'B' && h[q + 1] == 'C' && slen == 2 && q + 6 <= xend) bsize = (size_t)rd16(&h[q + 4]) + 1;
    q += 4 + slen;
  }
  if (bsize == 0 || bsize < xlen + 20) return false;
  *xlen_out = xlen;
  *bsize_out = bsize;
  return true;
}
// The block table of a BGZF file walked with pread: ONE read of a few dozen bytes per block -- the last four bytes of block k
// (ISIZE) and the header of block k + 1 lie next to each other -- and not a page of the file mapped for it.  emit(cpos, clen,
// upos, ulen, fpos) per block from file offset `from` on, until `until` (a block that STARTS at or behind it ends the walk) or
// the end of the file; *end = where the walk stopped.  false: no block header where one must be (*end says where).
template <class Emit>
static bool bgzf_walk_pread(int fd, size_t size, size_t from, size_t until, uint64_t upos, size_t max_blocks, size_t* end, Emit emit) {
  uint8_t h[4 + 256];
  size_t p = from, n = 0;
  if (p >= size || p >= until) { *end = p; return true; }
  ssize_t got = pread(fd, h + 4, 256, (off_t)p);
  while (true) {
    size_t xlen = 0, bsize = 0;
    if (got < 18 || !bgzf_parse_header(h + 4, (size_t)got, &xlen, &bsize) || p + bsize > size) { *end = p; return false; }
    // ISIZE of this block + the header of the next one
    got = pread(fd, h, 4 + 256, (off_t)(p + bsize - 4));
    if (got < 4) { *end = p; return false; }
    const uint32_t isize = rd32(h);
    emit(p + 12 + xlen, bsize - xlen - 20, upos, isize, p);
    upos += isize;
    p += bsize;
    ++n;
    got -= 4;
    if (p >= size || p >= until || n >= max_blocks) break;
  }
  *end = p;
  return true;
}

static bool bgzf_header_at(const uint8_t* c, size_t size, size_t p, size_t* xlen_out, size_t* bsize_out) {
  if (p + 18 > size || c[p] != 0x1f || c[p + 1] != 0x8b || c[p + 2] != 8 || !(c[p + 3] & 4)) return false;
  const size_t xlen = rd16(&c[p + 10]);
  size_t q = p + 12, xend = p + 12 + xlen, bsize = 0;
  while (q + 4 <= xend && xend <= size) {
    const uint16_t slen = rd16(&c[q + 2]);
    if (c[q] == 'B' && c[q + 1] == 'C' && slen == 2) bsize = (size_t)rd16(&c[q + 4]) + 1;
    q += 4 + slen;
  }
  if (bsize == 0 || p + bsize > size || bsize < xlen + 20) return false;
  *xlen_out = xlen;
  *bsize_out = bsize;
  return true;
}
// The first block start at or behind `from`: a header from which `chain` headers in a row follow one another (or the file ends
// behind fewer).  `size` when there is none.  (A guess: the caller's ranks compare their walks -- a rank's walk must END on the
// next rank's guess -- before any of them believes it.)
size_t bgzf_find_block(const uint8_t* c, size_t size, size_t from, int chain) {
  for (size_t p = from; p + 18 <= size && p < from + ((size_t)1 << 17); ++p) {
    if (c[p] != 0x1f || c[p + 1] != 0x8b) continue;
    size_t q = p;
    int ok = 0;
    while (ok < chain && q < size) {
      size_t xlen = 0, bsize = 0;
      if (!bgzf_header_at(c, size, q, &xlen, &bsize)) { ok = -1; break; }
      q += bsize;
      ++ok;
    }
    if (ok > 0) return p;
  }
  return size;
}

// A whole file's block table by several threads: thread k guesses the first block start behind k / T of the file (bgzf_find_block on
// the mapping: a few pages), walks with pread to thread k + 1's guess, and the pieces are believed only if every walk ENDS on the
// next one's guess -- else (a guess inside compressed bytes that looked like eight headers in a row) one thread walks it all.
// One thread spends 0.7 us a block on the two system calls: 0.25 s for a 9 GB BAM's 340 k blocks.
template <class Emit>
static bool bgzf_walk_file(int fd, const uint8_t* mapped, size_t size, size_t* end, uint64_t* total, Emit emit) {
  struct B { size_t cpos, clen; uint64_t upos; uint32_t ulen; size_t fpos; };
  const int budget = midas::cpu_budget();
  size_t least = (size_t)64 << 20;
  if (const char* e = getenv("MIDAS_SNPS_PARALLEL_WALK_MIN")) least = (size_t)strtoull(e, nullptr, 10);      // (tests: small files walked in pieces too)
  const int T = size < least || !mapped ? 1 : std::min(16, std::max(getenv("MIDAS_SNPS_PARALLEL_WALK_MIN") ? 4 : 1, budget));
  if (T > 1) {
    std::vector<size_t> start(T + 1, size);
    start[0] = 0;
    for (int k = 1; k < T; ++k) start[k] = bgzf_find_block(mapped, size, (size_t)((unsigned __int128)size * k / T), 8);
    bool sane = true;
    for (int k = 1; k <= T; ++k) sane = sane && start[k] > start[k - 1];
    if (sane) {
      std::vector<std::vector<B>> part(T);
      std::vector<size_t> stop(T, 0);
      std::vector<char> ok(T, 0);
      std::atomic<int> next{0};
      Workers::run(T, [&] {
        for (;;) {
          const int k = next.fetch_add(1);
          if (k >= T) return;
          part[k].reserve((start[k + 1] - start[k]) / 20000 + 16);
          size_t e = 0;
          ok[k] = bgzf_walk_pread(fd, size, start[k], start[k + 1], 0, ~(size_t)0, &e, [&](size_t cpos, size_t clen, uint64_t u, uint32_t ulen, size_t fpos) {
            part[k].push_back(B{cpos, clen, u, ulen, fpos});
          });
          stop[k] = e;
        }
      });
      bool chained = true;
      for (int k = 0; k < T; ++k) chained = chained && ok[k] && stop[k] == start[k + 1];
      if (getenv("MIDAS_SNPS_TRACE")) fprintf(stderr, "[bam inflate] block table walked in %d pieces: %s\n", T, chained ? "they chain" : "they do NOT chain (one thread walks it again)");
      if (chained) {
        uint64_t upos = 0;
        for (int k = 0; k < T; ++k) {
          for (const B& b : part[k]) emit(b.cpos, b.clen, upos + b.upos, b.ulen, b.fpos);
          if (!part[k].empty()) upos += part[k].back().upos + part[k].back().ulen;
        }
        *end = size;
        *total = upos;
        return true;
      }
    }
  }
  uint64_t upos = 0;
  const bool ok1 = bgzf_walk_pread(fd, size, 0, size, 0, ~(size_t)0, end, [&](size_t cpos, size_t clen, uint64_t u, uint32_t ulen, size_t fpos) {
    emit(cpos, clen, u, ulen, fpos);
    upos = u + ulen;
  });
  *total = upos;
  return ok1;
}

// A file mapping whose pages were touched goes in two steps: its pages are dropped piece by piece by several threads
// (MADV_DONTNEED takes the address space's lock SHARED: the pieces' page tables are emptied side by side, and the threads that
// are faulting elsewhere meanwhile -- the table writers, the genome reader -- are not held up as they are behind munmap's
// exclusive lock), then the empty range is unmapped.  munmap alone walks a 9 GB BAM's 2.2 M page-table entries on one core:
// 0.18 - 0.33 s on the GPU box.
static void pretouch_mapping(const uint8_t* base, size_t size) {
  (void)madvise(const_cast<uint8_t*>(base), size, MADV_WILLNEED);
  const size_t piece = (size_t)8 << 20, n_pieces = (size + piece - 1) / piece;
  const int n_workers = (int)std::min<size_t>(std::max<size_t>(n_pieces, 1), 16);
  std::atomic<size_t> nextp{0};
  std::atomic<unsigned> sink{0};
  Workers::run(n_workers, [&] {
    unsigned acc = 0;
    for (;;) {
      const size_t k = nextp.fetch_add(1);
      if (k >= n_pieces) break;
      const size_t end = std::min(size, (k + 1) * piece);
      for (size_t off = k * piece; off < end; off += 4096) acc += base[off];
    }
    sink += acc;
  });
}
static void unmap_file(const void* base, size_t size) {
  if (!base || !size) return;
  uint8_t* const b = static_cast<uint8_t*>(const_cast<void*>(base));
  const int budget = midas::cpu_budget();
  if (size >= ((size_t)256 << 20) && budget >= 2) {
    const size_t piece = (size_t)64 << 20, n_pieces = (size + piece - 1) / piece;
    const int nt = (int)std::min<size_t>(n_pieces, (size_t)std::min(budget, 16));
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;       // (threads of its own: the pool may be busy with the pileup's table writers)
    auto work = [&] {
      for (;;) {
        const size_t k = next.fetch_add(1);
        if (k >= n_pieces) return;
        const size_t lo = k * piece, hi = std::min(size, lo + piece);
        (void)madvise(b + lo, hi - lo, MADV_DONTNEED);
      }
    };
    for (int k = 1; k < nt; ++k) th.emplace_back(work);
    work();
    for (std::thread& t : th) t.join();
  }
  munmap(b, size);
}

void midas_hostio_unmap(const void* base, size_t size) { unmap_file(base, size); }

int32_t read_bgzf_file(const std::string& path, FileImage& comp, std::vector<FileBlk>& blocks, size_t* total, char* err256) {
  const int fd = open(path.c_str(), O_RDONLY);
  if (fd < 0) { set_err(err256, "cannot open %s", path.c_str()); return MIDAS_SNPS_ERR_INVALID_ARG; }
  struct stat sb;
  if (fstat(fd, &sb) != 0 || sb.st_size < 0) { close(fd); set_err(err256, "cannot stat %s", path.c_str()); return MIDAS_SNPS_ERR_INVALID_ARG; }
  const size_t fsz = (size_t)sb.st_size;
  Lap lap("bam inflate");
  const size_t piece = (size_t)8 << 20, n_pieces = (fsz + piece - 1) / piece;
  const int n_workers = (int)std::min<size_t>(std::max<size_t>(n_pieces, 1), 16);
  void* m = fsz > 0 && !getenv("MIDAS_SNPS_NO_MMAP") ? mmap(nullptr, fsz, PROT_READ, MAP_PRIVATE, fd, 0) : MAP_FAILED;
  bool mapped = false;
  if (m != MAP_FAILED) {
    // the WHOLE file is about to be read by this process (the host's inflater, or the upload's copy threads): its pages are
    // mapped in by several threads (one read per page: the kernel maps a run of cached pages per fault), the readers then find
    // them there.  The block table below is walked with pread all the same (bgzf_walk_file).
    comp.map = m;
    comp.p = static_cast<const uint8_t*>(m);
    comp.n = fsz;
    comp.fd = fd;
    pretouch_mapping(comp.p, fsz);
    mapped = true;
    lap("map file");
  } else {
    if (!comp.buf.resize(fsz)) { close(fd); set_err(err256, "out of memory reading %s", path.c_str()); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
    // the file comes in through several threads: one core copies ~4 GB/s out of the page cache, a BAM is 100s of MB
    std::atomic<size_t> nextp{0};
    std::atomic<int> short_read{0};
    uint8_t* const dst = comp.buf.data();
    Workers::run(n_workers, [&] {
      for (;;) {
        const size_t k = nextp.fetch_add(1);
        if (k >= n_pieces) return;
        size_t off = k * piece;
        const size_t end = std::min(fsz, off + piece);
        while (off < end) {
          const ssize_t got = pread(fd, dst + off, end - off, (off_t)off);
          if (got <= 0) { short_read = 1; return; }
          off += (size_t)got;
        }
      }
    });
    close(fd);
    if (short_read) { set_err(err256, "short read on %s", path.c_str()); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
    comp.p = comp.buf.data();
    comp.n = fsz;
    lap("read file");
  }
  size_t upos = 0;
  if (mapped) {
    size_t end = 0;
    uint64_t tot = 0;
    const bool ok = bgzf_walk_file(comp.fd, comp.p, fsz, &end, &tot, [&](size_t cpos, size_t clen, uint64_t u, uint32_t ulen, size_t fpos) {
      blocks.push_back({cpos, clen, u, ulen, fpos});
    });
    upos = (size_t)tot;
    if (!ok || end != fsz) { set_err(err256, "%s: not a BGZF block (or a truncated one) at offset %lld", path.c_str(), (long long)end); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
  } else {
  size_t p = 0;
  while (p < comp.size()) {
    if (p + 18 > comp.size() || comp[p] != 0x1f || comp[p + 1] != 0x8b || comp[p + 2] != 8 || !(comp[p + 3] & 4)) {
      set_err(err256, "%s: not a BGZF block at offset %lld", path.c_str(), (long long)p);
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
    const size_t xlen = rd16(&comp[p + 10]);
    size_t q = p + 12, xend = p + 12 + xlen;
    size_t bsize = 0;
    while (q + 4 <= xend) {
      const uint16_t slen = rd16(&comp[q + 2]);
      if (comp[q] == 'B' && comp[q + 1] == 'C' && slen == 2) bsize = (size_t)rd16(&comp[q + 4]) + 1;
      q += 4 + slen;
    }
    if (bsize == 0 || p + bsize > comp.size() || bsize < xlen + 20) {
      set_err(err256, "%s: truncated BGZF block at offset %lld", path.c_str(), (long long)p);
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
    const size_t isize = rd32(&comp[p + bsize - 4]);
    blocks.push_back({p + 12 + xlen, bsize - xlen - 20, upos, (uint32_t)isize, p});
    upos += isize;
    p += bsize;
  }
  }
  *total = upos;
  lap("block table");
  return MIDAS_SNPS_OK;
}

int32_t bgzf_inflate_file(const std::string& path, RawBuf<uint8_t>& out, char* err256, const midas::BlockInflater* inflater) {
  FileImage comp;
  std::vector<FileBlk> blocks;
  size_t upos = 0;
  {
    const int32_t rst = read_bgzf_file(path, comp, blocks, &upos, err256);
    if (rst != MIDAS_SNPS_OK) return rst;
  }
  typedef FileBlk Blk;
  Lap lap("bam inflate");
  if (!out.resize(upos)) { set_err(err256, "out of memory inflating %s", path.c_str()); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
  if (inflater) {
    std::vector<midas::InflateJob> jobs;
    jobs.reserve(blocks.size());
    for (const Blk& b : blocks) jobs.push_back({(uint64_t)b.cpos, (uint64_t)b.upos, (uint32_t)b.clen, (uint32_t)b.ulen, rd32(&comp[b.cpos + b.clen]), 1u});
    const midas::InflateSegment seg{comp.data(), comp.size()};
    int64_t bad_job = -1;
    const int32_t st = inflater->run(inflater->user, &seg, 1, jobs.data(), jobs.size(), out.data(), out.size(), &bad_job, err256);
    if (st == MIDAS_SNPS_ERR_BAD_LAYOUT)
      set_err(err256, "%s: corrupt BGZF block at file offset %lld (deflate data or CRC-32)", path.c_str(),
              (long long)(bad_job >= 0 && (size_t)bad_job < blocks.size() ? blocks[(size_t)bad_job].fpos : -1));
    lap("inflate blocks (inflater)");
    return st;
  }
  std::atomic<size_t> next{0};
  std::atomic<long long> bad{-1};
  auto work = [&] {
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= blocks.size()) return;
      const Blk& b = blocks[i];
      if (!bgzf_block_inflate(comp.data() + b.cpos, (size_t)b.clen, out.data() + b.upos, (size_t)b.ulen)) { bad = (long long)b.fpos; return; }
    }
  };
  const int nt = hw_threads(0);
  Workers::run(nt, work);
  lap("inflate blocks");
  if (bad >= 0) { set_err(err256, "%s: corrupt BGZF block at file offset %lld (deflate data or CRC-32)", path.c_str(), (long long)bad.load()); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
  return MIDAS_SNPS_OK;
}

// ---- a BAM mapped read-only, with its block table: the whole file's, or a rank's local one that grows along the chain ------
// walk a table's chain on from m.next_fpos, to `until` (a block that STARTS at or behind it ends the walk) or max_blocks further;
// false: no block header where one must be (m.next_fpos says where)
bool bgzf_walk_on(BgzfMap& m, size_t until, size_t max_blocks) {
  size_t end = m.next_fpos;
  const uint64_t upos = m.blocks.empty() ? 0 : m.blocks.back().upos + m.blocks.back().ulen;
  const bool ok = bgzf_walk_pread(m.fd, m.size, m.next_fpos, until, upos, max_blocks, &end, [&](size_t cpos, size_t clen, uint64_t u, uint32_t ulen, size_t fpos) {
    m.blocks.push_back({cpos, clen, u, ulen, fpos});
  });
  m.next_fpos = end;
  return ok;
}
// walk n_more blocks further along a local table's chain; false: the end of the file, or no block header where one must be
bool bgzf_grow(BgzfMap& m, size_t n_more) {     // (true: at least one block was added)
  const size_t before = m.blocks.size();
  (void)bgzf_walk_on(m, m.size, n_more);
  return m.blocks.size() > before;
}
// A file opened and mapped read-only into m (fd, size, base); what went wrong stays in m for its destructor.
int32_t map_file(const std::string& path, BgzfMap& m, char* err256) {
  m.fd = open(path.c_str(), O_RDONLY);
  if (m.fd < 0) { set_err(err256, "cannot open %s", path.c_str()); return MIDAS_SNPS_ERR_INVALID_ARG; }
  struct stat st;
  if (fstat(m.fd, &st) != 0) { set_err(err256, "cannot stat %s", path.c_str()); return MIDAS_SNPS_ERR_INVALID_ARG; }
  m.size = (size_t)st.st_size;
  if (m.size == 0) { set_err(err256, "%s is empty", path.c_str()); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
  void* a = mmap(nullptr, m.size, PROT_READ, MAP_PRIVATE, m.fd, 0);
  if (a == MAP_FAILED) { set_err(err256, "cannot map %s", path.c_str()); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
  m.base = static_cast<const uint8_t*>(a);
  return MIDAS_SNPS_OK;
}
int32_t bgzf_map_file(const std::string& path, BgzfMap& m, char* err256, bool touch) {
  const int32_t mst = map_file(path, m, err256);
  if (mst != MIDAS_SNPS_OK) return mst;
  // One caller that will read the WHOLE file (16 CPUs, one GPU): the pages are mapped in now, by several threads, and the
  // upload's threads copy out of the mapping (51 GB/s into the pinned ring on the GPU box; pread by as many threads: 33 GB/s).
  // A rank of N that takes 1 / N of the file, on the few CPUs a rank of N has: nothing is mapped in for it -- its upload reads
  // its share with pread (hostio.h, register_file_mapping), and there is no page table to take down afterwards.
  // (the pages are mapped in BESIDE the block table's walk, which reads the file with pread and looks into the mapping only for
  // its few guessed block starts: 57 + 30-70 ms one after the other at 9 GB)
  struct Toucher { std::thread t; ~Toucher() { if (t.joinable()) t.join(); } } toucher;
  if (touch) {
    const uint8_t* tb = m.base;
    const size_t ts = m.size;
    toucher.t = std::thread([tb, ts] { pretouch_mapping(tb, ts); });
  } else {
    midas::register_file_mapping(m.base, m.size, m.fd);
  }
  size_t end = 0;
  uint64_t upos = 0;
  const bool ok = bgzf_walk_file(m.fd, m.base, m.size, &end, &upos, [&](size_t cpos, size_t clen, uint64_t u, uint32_t ulen, size_t fpos) {
    m.blocks.push_back({cpos, clen, u, ulen, fpos});
  });
  if (!ok || end != m.size) {
    set_err(err256, "%s: not a BGZF block (or a truncated one) at offset %lld", path.c_str(), (long long)end);
    return MIDAS_SNPS_ERR_BAD_LAYOUT;
  }
  m.total = upos;
  m.next_fpos = m.size;
  return MIDAS_SNPS_OK;
}
