// Host-side I/O of the pileup stage, native because it bounds the end-to-end time once the kernel is fast:
//   * BAM (BGZF) decode into the BAM-native SoA the C-ABI takes      (reference: pysam.AlignmentFile + htslib
//     record decode, midas/run/snps.py:186; `samtools index` is not needed: the device indexes)
//   * <species>.snps.gz row formatter + multi-member gzip writer      (reference: midas/run/snps.py:179-182,
//     201-210 and utility.iopen, midas/utility.py:194-206)
// No GPU involved; exported through the same C-ABI library (include/midas_snps.h, "host I/O" section).
// This header: what the host I/O sources share (bgzf_host.cpp, bam_host.cpp, bam_shares.cpp, bam_writer.cpp, tables_host.cpp,
// fasta_host.cpp).  Whatever owns state is declared here and defined in one of them.
#pragma once
#include "hostio.h"
#include "row_deflate.h"
#include "workers.h"
#include "bam_parse.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/uio.h>
#include <unistd.h>
#include <dlfcn.h>
#include <zlib.h>

#include <algorithm>
#include <memory>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// A byte/word buffer that is NOT zero-filled when it grows: the BAM stream, its inflated form and the decoded SEQ / QUAL /
// CIGAR columns are hundreds of MB that get overwritten in full right away (std::vector::resize would memset them on one
// core first: a third of the decode time).
template <class T>
struct RawBuf {
  T* p = nullptr;
  size_t n = 0;
  RawBuf() = default;
  RawBuf(const RawBuf&) = delete;
  RawBuf& operator=(const RawBuf&) = delete;
  RawBuf(RawBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  ~RawBuf() { free(p); }
  bool resize(size_t m) {
    free(p);
    p = nullptr;
    const size_t bytes = m * sizeof(T);
    if (bytes >= ((size_t)8 << 20)) {
      // hundreds of MB that are written once, front to back: 2 MiB pages cut the first-touch faults 512-fold where
      // the kernel hands them out on request (transparent_hugepage = madvise)
      void* q = nullptr;
      if (posix_memalign(&q, (size_t)2 << 20, bytes) == 0) {
        (void)madvise(q, bytes, MADV_HUGEPAGE);
        p = static_cast<T*>(q);
      }
    } else if (m) {
      p = static_cast<T*>(malloc(bytes));
    }
    n = p ? m : 0;
    return m == 0 || p != nullptr;
  }
  void release() { free(p); p = nullptr; n = 0; }
  T* data() { return p; }
  const T* data() const { return p; }
  size_t size() const { return n; }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
};

// A BAM file mapped read-only with its BGZF block table (rank-local decode: a rank inflates only the blocks it needs).
void midas_hostio_unmap(const void* base, size_t size);      // (a file mapping taken down by several threads: defined below)
struct BgzfMap {
  const uint8_t* base = nullptr;
  size_t size = 0;
  int fd = -1;
  struct Blk { size_t cpos, clen; uint64_t upos; uint32_t ulen; size_t fpos; };
  std::vector<Blk> blocks;
  uint64_t total = 0;          // uncompressed bytes
  // A rank's LOCAL table (midas_bam_open_share_local): `blocks` begins at the first block of the rank's share of the file's
  // bytes, not at the file's; the chain goes on at next_fpos when somebody asks beyond it (grow).  A whole table: next_fpos == size.
  size_t next_fpos = 0;
  bool local = false;
  // (bgzf_grow(map, n): walk n blocks further along the chain)
  size_t block_holding(uint64_t u) const { return midas::block_holding(blocks.data(), blocks.size(), u); }        // (bam_parse.h)
  size_t first_block_at(size_t at) const { return midas::first_block_at(blocks.data(), blocks.size(), at); }
  ~BgzfMap() {
    if (base && size) { midas::unregister_file_mapping(base); midas_hostio_unmap(base, size); }
    if (fd >= 0) close(fd);
  }
};

struct midas_bam {
  // rank-local mode (midas_bam_open_slice): the mapped file and what the walk over this rank's slice found
  std::unique_ptr<BgzfMap> map;
  int64_t slice_first = -1, slice_end = -1;   // uncompressed offsets: first record starting in the slice / first one behind it
  int32_t slice_sorted = 1, slice_first_ref = -1, slice_last_ref = -1;
  std::vector<int64_t> ref_reads, ref_bases, ref_first;
  // for cutting long references into pieces (midas_bam_slice_marks): positions sorted inside every reference so far, the
  // first / last record's position, every reference's longest read span on it, and {refID, pos / MIDAS_BAM_MARK_SPAN,
  // offset} of the first record of every (reference, position bin > 0) met
  int32_t slice_pos_sorted = 1;
  int64_t slice_first_pos = -1, slice_last_pos = -1;
  std::vector<int64_t> ref_span, marks;
  std::string path;
  std::vector<std::string> ref_names;
  std::vector<int64_t> ref_lens;
  RawBuf<uint8_t> data;        // inflated stream
  size_t rec_begin = 0;        // offset of the first alignment record
  // decoded SoA
  RawBuf<int32_t> refid, pos, nm, l_seq;
  RawBuf<uint8_t> mapq;
  RawBuf<uint8_t> seq4, qual;
  RawBuf<uint16_t> flag;
  RawBuf<int64_t> seq_off, qual_off, cigar_off;   // n + 1 entries each
  RawBuf<uint32_t> cigar;
  size_t n_records = 0;
  bool loaded = false;
  // midas_bam_load_device: SEQ / QUAL / CIGAR are cut out of the inflated stream ON THE DEVICE and stay there (the columns
  // call hands out device pointers for them); the host decodes everything else
  bool payload_on_device = false;
  std::vector<uint64_t> rec_off;        // where every decoded record starts in the inflated stream (kept for the device's cut)
  void* dev_payload[3] = {nullptr, nullptr, nullptr};
  void* dev_owner = nullptr;            // the device allocation the three live in
  void (*dev_free)(void*) = nullptr;
  // midas_bam_load_resident: EVERY column stays on the device, the records also in the pileup kernel's own layout; only refID is
  // in host memory.  midas_bam_resident_to_columns turns the handle into the payload_on_device form above (and keeps this).
  bool resident = false;
  midas::ResidentReads rr;
  int64_t rr_seq_bytes = 0, rr_qual_bytes = 0, rr_n_cigar = 0;
  void* dev_owner2 = nullptr;           // (the three payload columns cut later, in a buffer of their own)
  void (*dev_free2)(void*) = nullptr;
  ~midas_bam() {
    if (dev_free2 && dev_owner2) dev_free2(dev_owner2);
    if (dev_free && dev_owner) dev_free(dev_owner);
  }
};

namespace {

using midas::Workers;
using midas::plausible_bytes;

void set_err(char* err256, const char* fmt, const char* a = "", long long b = 0) {
  if (err256) snprintf(err256, 256, fmt, a, b);
}

inline uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint16_t rd16(const uint8_t* p) { uint16_t v; memcpy(&v, p, 2); return v; }

int hw_threads(int want) {
  unsigned n = (unsigned)midas::cpu_budget();      // hardware threads, or the cgroup's CPU quota when that is less
  if (want > 0) n = std::min<unsigned>(n, (unsigned)want);
  if (n > 128) n = 128;
  return (int)n;
}

// Threads of the row writer: the caller's --threads when given, else every core (capped at 128; 256 SMT threads
// measured no faster on a 128-core host, 0.21 vs 0.23-0.29 s with zlib).
#ifndef MIDAS_WRITER_MAX_THREADS
#define MIDAS_WRITER_MAX_THREADS 128
#endif
int writer_threads(int want) {
  unsigned n = (unsigned)midas::cpu_budget();
  if (want > 0) n = std::min<unsigned>(n, (unsigned)want);
  if (n > MIDAS_WRITER_MAX_THREADS) n = MIDAS_WRITER_MAX_THREADS;
  return (int)n;
}

// Developer variants (-DMIDAS_HOSTIO_TRACE): where the host stages spend their time, on stderr.
struct Lap {       // where a call spends its time, on stderr, when MIDAS_SNPS_TRACE is set
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  const char* who;
  bool on;
  explicit Lap(const char* w) : who(w), on(getenv("MIDAS_SNPS_TRACE") != nullptr) {}
  void operator()(const char* what) {
    if (!on) return;
    const auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "[%s] %-34s %8.2f ms\n", who, what, std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  }
};

// decimal formatting of a u32 into buf (returns new end)
inline char* put_u32(char* p, uint32_t v) {
  char tmp[10];
  int n = 0;
  do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
  while (n) *p++ = tmp[--n];
  return p;
}
inline char* put_u64(char* p, uint64_t v) {
  char tmp[20];
  int n = 0;
  do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
  while (n) *p++ = tmp[--n];
  return p;
}

template <class F>
void run_pool(int nt, size_t n_tasks, F&& fn) {
  std::atomic<size_t> next{0};
  auto work = [&] {
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= n_tasks) return;
      fn(i);
    }
  };
  if ((size_t)nt > n_tasks) nt = (int)std::max<size_t>(1, n_tasks);
  Workers::run(nt, work);
}

}  // namespace

// ---- shared between the sources, and not part of the library's surface ---------------------------------------------------------
#pragma GCC visibility push(hidden)

// One raw DEFLATE stream of known inflated size (a BGZF block, a member of one of this library's tables) -> out.  Through
// libdeflate when the system has it (looked up once with dlopen -- it is what htslib itself prefers, and two to three times
// zlib's speed on BAM blocks), else zlib.  MIDAS_SNPS_INFLATE=zlib keeps it to zlib.
struct Libdeflate {
  void* (*alloc)() = nullptr;
  int (*run)(void*, const void*, size_t, void*, size_t, size_t*) = nullptr;
  void (*release)(void*) = nullptr;
  uint32_t (*crc)(uint32_t, const void*, size_t) = nullptr;
  Libdeflate() {
    const char* pick = getenv("MIDAS_SNPS_INFLATE");
    if (pick && strcmp(pick, "zlib") == 0) return;
    void* h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
    void* a = dlsym(h, "libdeflate_alloc_decompressor");
    void* r = dlsym(h, "libdeflate_deflate_decompress");
    void* f = dlsym(h, "libdeflate_free_decompressor");
    void* c = dlsym(h, "libdeflate_crc32");
    if (!a || !r || !f) return;
    if (c) crc = reinterpret_cast<uint32_t (*)(uint32_t, const void*, size_t)>(c);
    alloc = reinterpret_cast<void* (*)()>(a);
    run = reinterpret_cast<int (*)(void*, const void*, size_t, void*, size_t, size_t*)>(r);
    release = reinterpret_cast<void (*)(void*)>(f);
  }
};
const Libdeflate& libdeflate();                                                   // (bgzf_host.cpp: looked up once)
bool raw_inflate(const uint8_t* in, size_t n_in, uint8_t* out, size_t n_out);     // (bgzf_host.cpp: a decompressor per thread)
namespace {

// CRC-32 (gzip's) of a buffer: libdeflate's (carry-less multiplication, tens of GB/s a core) when it is there, else zlib's.
uint32_t crc32_of(const uint8_t* p, size_t n) {
  const Libdeflate& l = libdeflate();
  if (l.crc) return l.crc(0u, p, n);
  return (uint32_t)crc32(crc32(0L, Z_NULL, 0), p, (uInt)n);
}
// A BGZF block: its stream inflated to exactly n_out bytes AND those bytes' CRC-32 equal to the one stored behind the stream
// (what htslib's bgzf_read_block checks behind pysam.AlignmentFile, midas/run/snps.py:186).  false: corrupt, one way or the other.
bool bgzf_block_inflate(const uint8_t* in, size_t n_in, uint8_t* out, size_t n_out) {
  if (!raw_inflate(in, n_in, out, n_out)) return false;
  return crc32_of(out, n_out) == rd32(in + n_in);
}

}  // namespace

typedef BgzfMap::Blk FileBlk;
// A BGZF file read whole (by several threads) and its block table: where every block's DEFLATE stream lies, what it inflates to.
// A whole file's bytes for reading: the file MAPPED where that works (a BAM of a gigabyte is in the page cache when the pileup
// stage starts -- bowtie2 | samtools just wrote it; copying it into a fresh buffer costs a first-touch fault and a copy per
// page, 90 ms a gigabyte on the GPU box, mapping it 10) -- else read into a buffer by several threads.
struct FileImage {
  const uint8_t* p = nullptr;
  size_t n = 0;
  void* map = nullptr;
  int fd = -1;
  RawBuf<uint8_t> buf;
  FileImage() = default;
  FileImage(const FileImage&) = delete;
  FileImage& operator=(const FileImage&) = delete;
  ~FileImage() {
    if (map) { midas::unregister_file_mapping(map); midas_hostio_unmap(map, n); }
    if (fd >= 0) close(fd);
  }
  const uint8_t* data() const { return p; }
  size_t size() const { return n; }
  const uint8_t& operator[](size_t i) const { return p[i]; }
};

// bgzf_host.cpp
int32_t read_bgzf_file(const std::string& path, FileImage& comp, std::vector<FileBlk>& blocks, size_t* total, char* err256);
int32_t bgzf_inflate_file(const std::string& path, RawBuf<uint8_t>& out, char* err256, const midas::BlockInflater* inflater = nullptr);
size_t bgzf_find_block(const uint8_t* c, size_t size, size_t from, int chain);
bool bgzf_walk_on(BgzfMap& m, size_t until, size_t max_blocks);
bool bgzf_grow(BgzfMap& m, size_t n_more);
int32_t map_file(const std::string& path, BgzfMap& m, char* err256);
int32_t bgzf_map_file(const std::string& path, BgzfMap& m, char* err256, bool touch = true);

// Inflated bytes of the consecutive blocks [b_lo, b_hi) of a mapped BAM; grows at the far end on demand.
struct BamWindow {
  const BgzfMap* m = nullptr;
  BgzfMap* growable = nullptr;      // (a rank's local table: the window walks the chain on when it needs blocks behind the table's last)
  size_t b_lo = 0, b_hi = 0;
  std::vector<uint8_t> buf;
  std::atomic<long long> bad_fpos{-1};      // (extend: the file offset of a block that did not inflate)
  uint64_t u_lo() const { return b_lo < m->blocks.size() ? m->blocks[b_lo].upos : m->total; }
  uint64_t u_hi() const { return u_lo() + buf.size(); }
  bool extend(size_t new_hi) {   // inflate blocks [b_hi, new_hi) behind what is there
    if (growable && new_hi > m->blocks.size()) (void)bgzf_grow(*growable, new_hi - m->blocks.size());
    if (new_hi > m->blocks.size()) new_hi = m->blocks.size();
    if (new_hi <= b_hi) return true;
    size_t add = 0;
    for (size_t i = b_hi; i < new_hi; ++i) add += m->blocks[i].ulen;
    const size_t old = buf.size();
    buf.resize(old + add);
    std::vector<size_t> at(new_hi - b_hi);
    size_t o = old;
    for (size_t i = b_hi; i < new_hi; ++i) { at[i - b_hi] = o; o += m->blocks[i].ulen; }
    std::atomic<int> bad{0};
    const size_t first = b_hi;
    run_pool(hw_threads(0), new_hi - b_hi, [&](size_t k) {
      const BgzfMap::Blk& b = m->blocks[first + k];
      if (!bgzf_block_inflate(m->base + b.cpos, (size_t)b.clen, buf.data() + at[k], (size_t)b.ulen)) { bad = 1; bad_fpos = (long long)b.fpos; }
    });
    b_hi = new_hi;
    return bad == 0;
  }
  // make bytes [u, u + n) available (n bytes from uncompressed offset u >= u_lo()); false at end of file / bad data
  bool need(uint64_t u, size_t n) {
    while (u + n > u_hi()) {
      if (b_hi >= m->blocks.size() && !(growable && bgzf_grow(*growable, 4))) return false;
      if (!extend(b_hi + 4)) return false;
    }
    return true;
  }
  const uint8_t* at(uint64_t u) const { return buf.data() + (u - u_lo()); }
};

// bam_host.cpp
int32_t read_bam_header(BamWindow& w, midas_bam* b, const char* corrupt_fmt, char* err256);
int32_t decode_records(midas_bam* b, const uint8_t* d, const std::vector<size_t>& offs, char* err256, const uint32_t* heads = nullptr);
bool alloc_host_columns(midas_bam* b, int64_t n, midas::HostColumns* c, bool keep_refid = false);
void adopt_device_result(midas_bam* b, const midas::DeviceDecodeResult& res, int payload);
// The columns a device decode brings down, in the handle's own buffers (payload == 2: refID alone); ok = false: out of memory.
struct ColumnSink {
  midas_bam* b; bool ok; int payload;
  static midas::HostColumns alloc(void* sink, int64_t n);
};
void set_decode_error(char* err256, const char* path, long long bad_fpos, int64_t bad_record, const char* otherwise);
inline void report_totals(int64_t n, int64_t seq, int64_t qual, int64_t cigar, int64_t* n_reads, int64_t* seq_bytes, int64_t* qual_bytes, int64_t* n_cigar) {
  if (n_reads) *n_reads = n;
  if (seq_bytes) *seq_bytes = seq;
  if (qual_bytes) *qual_bytes = qual;
  if (n_cigar) *n_cigar = cigar;
}
#pragma GCC visibility pop
