// merge_rows.hip for the translation units that use it (merge_sites.hip): the rows of snps_freq.txt / snps_depth.txt formatted on
// the device from the arrays the merge kernel leaves there, and the text's way down through the context's pinned ring into files.
#pragma once
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "ctx_internal.h"

namespace midas {

// A table on its way to disk: written under <path>.tmp.<pid>, renamed by commit(); whatever happens before that leaves nothing
// under the final name (the destructor removes the temporary file).
struct MergeTextFile {
  std::string path, tmp;
  int fd = -1;
  long long off = 0;            // where the next bytes go: the device side hands the offsets out, the writer thread pwrites there
  bool open(const char* final_path, const char* header_line);
  bool commit();
  ~MergeTextFile();
};

// The file side of the ring: ONE thread that writes the slots the device side has filled, in the order they were filled, each
// at the file offset that came with it (pwrite), while the device side formats and copies the next ones.  (Several writers into
// one file were measured slower: profiles/merge_snps_e2e.txt.)  The caller holds the context's copy_mutex for as long as a MergeTextSink lives.
class MergeTextSink {
 public:
  explicit MergeTextSink(midas_snps_ctx* ctx);
  ~MergeTextSink();
  int32_t start();                                              // the ring's slots, the thread
  // n bytes of device memory into `to`, through the ring, in order after everything sent before
  int32_t send(MergeTextFile* to, const uint8_t* d_text, size_t n);
  bool finish();                                                // waits for the writes; false: a write failed
  double copy_s = 0, write_s = 0;                               // the copies down (device side), the file writes (the thread)
  long long bytes = 0;

 private:
  void run();
  midas_snps_ctx* ctx_;
  std::thread thread_;
  std::mutex m_;
  std::condition_variable cv_;
  struct Slot { MergeTextFile* to = nullptr; size_t n = 0; long long off = 0; bool full = false; } slot_[midas_snps_ctx::kStageSlots];
  unsigned long long sent_ = 0, written_ = 0;
  bool stop_ = false, failed_ = false, started_ = false;
};

// The formatter of one call: device buffers sized once for the call's number of samples and its largest chunk.
class MergeRowFormatter {
 public:
  MergeRowFormatter(midas_snps_ctx* ctx, int32_t n_samples) : ctx_(ctx), n_samples_(n_samples) {}
  ~MergeRowFormatter();
  // buffers for chunks of up to max_rows kept rows; with_compact: those of compact() too
  int32_t prepare(long long max_rows, bool with_compact);
  // The kept sites of a chunk from the calls word the merge kernel wrote (flag byte == 0), in site order: *d_keep (owned by
  // the formatter, valid until the next call), *n_keep.  Waits for the stream.
  int32_t compact(const uint32_t* d_calls, uint32_t m, const uint32_t** d_keep, long long* n_keep);
  // One table's rows for the kept sites d_keep[0, n_keep) (indices into the chunk's m sites) -> sink -> file.  d_minor == nullptr:
  // the depth table.  Row r carries site id id_base + d_keep[r] + 1.  A minor count above its depth: INVALID_ARG.
  int32_t emit(const uint32_t* d_depth, const uint32_t* d_minor, uint32_t m, const uint32_t* d_keep, long long n_keep,
               long long id_base, MergeTextSink* sink, MergeTextFile* to);
  float format_ms = 0.f;                                        // the formatter's kernels (HIP events)

 private:
  midas_snps_ctx* ctx_;
  int32_t n_samples_;
  long long max_rows_ = 0;
  size_t text_cap_ = 0, text_bytes_ = 0;
  uint32_t* d_len_ = nullptr;        // [rows of a batch + 1]: lengths, then (scanned) where the rows start
  uint32_t* d_rank_ = nullptr;       // [max_rows + 1]  (compact() only)
  uint32_t* d_keep_ = nullptr;       // [max_rows]      (compact() only)
  uint32_t* d_scratch_ = nullptr;
  uint8_t* d_text_ = nullptr;
  unsigned long long* d_err_ = nullptr;
  unsigned long long* h_down_ = nullptr;      // page-locked: a batch's total and error word
  hipEvent_t e0_ = nullptr, e1_ = nullptr;
};

}  // namespace midas
