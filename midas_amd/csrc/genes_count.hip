// `run_midas.py genes` on MI355X: count_mapped_bp (/root/reference/midas/run/genes.py:165-189) -- for every gene of the
// pangenome, how many reads align to it, how many pass keep_read (:148-163, the same predicate as the snps path), and
// the gene's depth = sum over kept reads of len(query_alignment_sequence) / float(gene.length).
//
// The reference walks the (unsorted) BAM once and accumulates `gene.depth += align_len / float(gene.length)` read by
// read.  fp64 addition is not associative, so the sum has to be reproduced in exactly that order:
//   facts   per read, 8 bytes: aligned length (pysam's clip rules), l_seq, NM, floor(mean quality), mapq, three
//           "absent" flags -- a pass over the quality bytes and CIGARs: on all host cores when those columns are host
//           memory (pack_records), by sixteen lanes a read when they lie on the device (genes_facts_kernel,
//           midas_genes_count_device: what midas_sam_load_device_order / midas_bam_load_device hand out);
//   filter  one thread per read, BAM order: keep_read with the exceptions the reference would raise (lowest read
//           index wins), and the read's term  align_len / float(gene.length)  (+0.0 for a read that is dropped:
//           adding it leaves the running sum unchanged bit for bit);
//   sort    stable LSD radix sort of (gene, term) pairs by gene, eight bits of the gene index a pass (device_sort.hip, the
//           library's own: a gene index has as many bits as the pangenome has genes): BAM order survives inside a gene;
//   bounds  first sorted position of every gene;
//   sum     one thread per gene adds its terms one after the other (a gene with many reads: one wave stages 512
//           terms at a time in LDS and adds them in the same order).
// Genes are independent, so the device parallelism of the last step is over genes (10^5 - 10^6 per sample).
//
// N ranks (run/genes.py): the two halves are entry points of their own -- midas_genes_terms (host + filter: a rank's slice of
// the BAM -> one term per read) and midas_genes_sum (sort + bounds + sum over the pairs a gene's owner received, which arrive
// in BAM order) -- so that a gene's running sum is formed on ONE rank in the order the reference forms it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/midas_snps.h"
#include "ctx_internal.h"
#include "workers.h"
#include "device_common.h"
#include "kernels.h"
#include "bam_record.h"

namespace midas {
namespace {

// word 0: align_len (11) | l_seq (11) << 11 | flags (3) << 22      word 1: NM (16) | qmean (8) << 16 | mapq (8) << 24
// qmean = floor(mean(query_qualities)): np.mean(q) < readq  <=>  qmean < readq for an integer readq
constexpr uint32_t kNoSeq = 1, kNoNm = 2, kNoQual = 4;
constexpr int kHeavyGene = 2048;       // reads; genes above it are summed by a whole wave

struct FilterKParams {
  const uint2* rec;              // [n] BAM order
  const uint32_t* gene;          // [n] reference id = gene index
  const int64_t* gene_len;       // [n_genes]
  const FilterTables* filt;
  double* term;                  // [n] out
  unsigned long long* err;       // atomicMin((read << 8) | kind)
  long long n;
  int mapq, readq;
};

__global__ __launch_bounds__(256) void genes_filter_kernel(FilterKParams p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  const uint2 r = p.rec[i];
  const int align_len = (int)(r.x & 2047u), l_seq = (int)((r.x >> 11) & 2047u);
  const uint32_t flags = r.x >> 22;
  const int nm = (int)(r.y & 0xFFFFu), qmean = (int)((r.y >> 16) & 0xFFu), mapq = (int)(r.y >> 24);
  // keep_read (genes.py:148-163): identity, mean quality, mapping quality, aligned fraction -- in that order, with
  // the exceptions the reference would raise in the order it would raise them
  uint32_t err = 0;
  bool keep = false;
  if (flags & kNoSeq) err = dev::E_NO_SEQ;                           // len(None)
  else if (flags & kNoNm) err = dev::E_NO_NM;                        // dict(aln.tags)['NM']
  else if (align_len == 0) err = dev::E_ZERO_ALIGN;                  // / float(0)
  else if (align_len - nm < p.filt->min_match[align_len]) keep = false;
  else if (flags & kNoQual) err = dev::E_NO_QUAL;                    // np.mean(None)
  else if (qmean < p.readq) keep = false;
  else if (mapq < p.mapq) keep = false;
  else if (align_len < p.filt->min_align[l_seq]) keep = false;
  else keep = true;
  if (err) atomicMin(p.err, ((unsigned long long)i << 8) | err);
  // the reference's own expression; a dropped read contributes +0.0
  p.term[i] = keep ? (double)align_len / (double)p.gene_len[p.gene[i]] : 0.0;
}

// ---- the 8-byte record from DEVICE-resident QUAL / CIGAR columns: pack_records, to the bit ---------------------------------
// A read's record is made by sixteen lanes (a quarter wave).  Its quality run [q0, q0 + l) starts at any byte: lane k takes
// the 16-byte ALIGNED granules k, k + 16, ... of the run (one global_load_dwordx4 each, 256 contiguous bytes a read and
// step), drops the bytes in front of and behind the run with a byte mask, and adds the rest up four at a time (v_sad_u8
// against zero).  A granule that is not wholly inside the column [qual, qual + qual_total) -- only a run's first one when
// the column starts off a 16-byte border, only its last one when the column ends there (the last read's) -- is not loaded
// as a vector: its at most 15 bytes of the run are fetched one by one, so no load reaches outside the column whatever its
// address and whatever lies behind it.  The partial sums meet by four xor-shuffles inside the quarter wave.  Lane 0 walks
// the few CIGAR ops at both ends and stores the record (one 8-byte store).
// A read pack_records would refuse leaves (read << 8 | kind) in *bad, lowest read first, and a record of zeros; its gene is
// set to 0 so that the filter kernel behind this one indexes nothing outside the gene table.  Offsets that point outside
// their column are refused here too (kFactLayout): the host's pass would read whatever lies there, a kernel must not.
enum : uint32_t { kFactRef = 1, kFactLayout = 2, kFactSize = 3, kFactRecord = 4 };      // (kFactRecord: bam_genes_facts_kernel's alone)
constexpr int kFactLanes = 16;

struct FactsKParams {
  const int32_t* l_seq; const int32_t* nm; const uint8_t* mapq;      // [n]
  const long long* qual_off; const long long* cigar_off;             // [n + 1]
  const uint8_t* qual; const uint32_t* cigar;                        // the columns, qual_total bytes / cigar_total ops
  long long qual_total, cigar_total;
  uint32_t* gene;                // [n] in: ref_id; a gene outside the table becomes 0
  uint2* rec;                    // [n] out
  unsigned long long* bad;       // atomicMin((read << 8) | kind)
  long long n, n_genes;
};

__device__ __forceinline__ uint32_t byte_mask4(uint32_t nib) {      // bit k of nib -> byte k all ones
  return ((nib & 1u) | (nib & 2u) << 7 | (nib & 4u) << 14 | (nib & 8u) << 21) * 0xFFu;
}

__global__ __launch_bounds__(256) void genes_facts_kernel(FactsKParams p) {
  const int sub = threadIdx.x & (kFactLanes - 1);
  const long long i = (long long)blockIdx.x * (256 / kFactLanes) + (threadIdx.x / kFactLanes);
  if (i >= p.n) return;                               // (the same in all sixteen lanes of a read, like everything up to the loads)
  const long long g = (long long)(int32_t)p.gene[i];
  const long long l = p.l_seq[i], nm = p.nm[i];
  const long long q0 = p.qual_off[i], q1 = p.qual_off[i + 1], c0 = p.cigar_off[i], c1 = p.cigar_off[i + 1];
  const long long nc = c1 - c0;
  uint32_t kind = 0;
  if (g < 0 || g >= p.n_genes) kind = kFactRef;
  else if (l < 0 || nc < 0 || q1 - q0 < l || q0 < 0 || q0 + l > p.qual_total || c0 < 0 || c1 > p.cigar_total) kind = kFactLayout;
  else if (l > kMaxLSeq || nm > kMaxField16) kind = kFactSize;
  if (kind) {
    if (sub == 0) {
      atomicMin(p.bad, ((unsigned long long)i << 8) | kind);
      p.rec[i] = make_uint2(0u, 0u);
      if (kind == kFactRef) p.gene[i] = 0u;
    }
    return;
  }
  // ---- sum of the l quality bytes ------------------------------------------------------------------------------------------
  const unsigned long long col_lo = (unsigned long long)p.qual, col_hi = col_lo + (unsigned long long)p.qual_total;
  const unsigned long long run_lo = col_lo + (unsigned long long)q0, run_hi = run_lo + (unsigned long long)l;
  uint32_t qsum = 0;
  for (unsigned long long b = (run_lo & ~15ull) + 16ull * (unsigned)sub; b < run_hi; b += 16ull * kFactLanes) {
    const unsigned long long lo = b < run_lo ? run_lo : b, hi = b + 16 > run_hi ? run_hi : b + 16;     // the run's bytes of this granule
    if (b >= col_lo && b + 16 <= col_hi) {
      const uint4 v = *reinterpret_cast<const uint4*>(p.qual + (b - col_lo));        // (off the column's pointer: a global load)
      const uint32_t m = ((1u << (unsigned)(hi - b)) - 1u) & ~((1u << (unsigned)(lo - b)) - 1u);         // (hi - b <= 16)
      qsum = __builtin_amdgcn_sad_u8(v.x & byte_mask4(m & 15u), 0u, qsum);
      qsum = __builtin_amdgcn_sad_u8(v.y & byte_mask4((m >> 4) & 15u), 0u, qsum);
      qsum = __builtin_amdgcn_sad_u8(v.z & byte_mask4((m >> 8) & 15u), 0u, qsum);
      qsum = __builtin_amdgcn_sad_u8(v.w & byte_mask4((m >> 12) & 15u), 0u, qsum);
    } else {
      for (unsigned long long a = lo; a < hi; ++a) qsum += p.qual[a - col_lo];          // (a column's border granule: < 16 bytes)
    }
  }
#pragma unroll
  for (int w = kFactLanes / 2; w >= 1; w >>= 1) qsum += (uint32_t)__shfl_xor((int)qsum, w, kFactLanes);
  if (sub != 0) return;
  // ---- [EXT] pysam query_alignment_start / _end, as pack_records walks them -----------------------------------------------------
  const uint32_t* cg = p.cigar + c0;
  long long qs = 0;
  for (long long k = 0; k < nc; ++k) {
    const uint32_t w = cg[k], op = w & 15u;
    if (op == 5u) continue;
    if (op == 4u) qs += w >> 4; else break;
  }
  long long qe = l;
  for (long long k = nc - 1; k >= 1; --k) {
    const uint32_t w = cg[k], op = w & 15u;
    if (op == 5u) continue;
    if (op == 4u) qe -= w >> 4; else break;
  }
  long long al = qe - qs > 0 ? qe - qs : 0;
  if (al > l) al = l;
  const bool no_qual = l > 0 && p.qual[q0] == 0xFFu;
  const uint32_t flags = (l == 0 ? kNoSeq : 0u) | (nm < 0 ? kNoNm : 0u) | (no_qual ? kNoQual : 0u);
  const uint32_t nm_u = (uint32_t)(nm < 0 ? 0 : nm);
  const uint32_t qmean = l > 0 ? qsum / (uint32_t)l : 0u;
  p.rec[i] = make_uint2((uint32_t)al | ((uint32_t)l << 11) | (flags << 22), nm_u | (qmean << 16) | ((uint32_t)p.mapq[i] << 24));
}

// ---- the 8-byte record straight from the alignment RECORD where it lies in the inflated BAM stream (midas_genes_count_bam) ----------
// The same sixteen lanes a read, the same granule scheme -- the "column" is the whole stream d[0, total), a record starts at any byte
// of it, and its QUAL run lies at r + 36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2.  Only the stream's own first and last
// granule can fail to lie wholly inside it; those are fetched byte by byte, so no load reaches outside [d, d + total) whatever
// follows the stream in the arena.  Lane 0 walks the CIGAR ends in the record ([EXT], as above) and finds NM in its aux block
// (bam_record.h find_nm, the one bam_columns_kernel uses).  Nothing was cut into columns for this and nothing per read comes down.
// Refused, lowest read first, with a record of zeros: a record whose variable parts overrun its block_size or whose refID names no
// reference (kFactRecord: what bam_columns_kernel calls bad_record; the gene becomes 0), l_seq or NM beyond the record (kFactSize).
struct BamFactsKParams {
  const uint8_t* d; unsigned long long total;      // the inflated stream
  const unsigned long long* rec_off;               // [n] the kept records (refID >= 0), file order (bam_offsets_kernel)
  uint32_t* gene;                                  // [n] out: refID
  uint2* rec;                                      // [n] out
  unsigned long long* bad;                         // atomicMin((read << 8) | kind)
  long long n, n_genes;
};

__global__ __launch_bounds__(256) void bam_genes_facts_kernel(BamFactsKParams p) {
  const int sub = threadIdx.x & (kFactLanes - 1);
  const long long i = (long long)blockIdx.x * (256 / kFactLanes) + (threadIdx.x / kFactLanes);
  if (i >= p.n) return;                               // (the same in all sixteen lanes of a read, like everything up to the loads)
  const unsigned long long u = p.rec_off[i];
  uint32_t kind = 0;
  uint32_t bs = 0, w3 = 0, n_cig = 0, l = 0;
  long long g = 0;
  unsigned long long body = 0;
  const uint8_t* r = p.d + u;
  if (u + 36ull > p.total) {                          // (the walk hands out no such offset: nothing is read through it all the same)
    kind = kFactRecord;
  } else {
    bs = rd32(r);
    g = (long long)(int32_t)rd32(r + 4);
    w3 = rd32(r + 12);
    n_cig = rd32(r + 16) & 0xFFFFu;
    l = rd32(r + 20);
    body = 32ull + (w3 & 0xFFu) + 4ull * n_cig + ((unsigned long long)l + 1ull) / 2ull + l;
    if (u + 4ull + bs > p.total || body > bs || g < 0 || g >= p.n_genes) kind = kFactRecord;
    else if (l > (uint32_t)kMaxLSeq) kind = kFactSize;
  }
  if (kind) {
    if (sub == 0) {
      atomicMin(p.bad, ((unsigned long long)i << 8) | kind);
      p.rec[i] = make_uint2(0u, 0u);
      p.gene[i] = kind == kFactRecord ? 0u : (uint32_t)g;
    }
    return;
  }
  const uint32_t lrn = w3 & 0xFFu;
  // ---- sum of the l quality bytes ------------------------------------------------------------------------------------------
  const unsigned long long col_lo = (unsigned long long)p.d, col_hi = col_lo + p.total;
  const unsigned long long q0 = u + 36ull + lrn + 4ull * n_cig + (l + 1u) / 2u;
  const unsigned long long run_lo = col_lo + q0, run_hi = run_lo + l;
  uint32_t qsum = 0;
  for (unsigned long long b = (run_lo & ~15ull) + 16ull * (unsigned)sub; b < run_hi; b += 16ull * kFactLanes) {
    const unsigned long long lo = b < run_lo ? run_lo : b, hi = b + 16 > run_hi ? run_hi : b + 16;     // the run's bytes of this granule
    if (b >= col_lo && b + 16 <= col_hi) {
      const uint4 v = *reinterpret_cast<const uint4*>(p.d + (b - col_lo));           // (off the stream's pointer: a global load)
      const uint32_t m = ((1u << (unsigned)(hi - b)) - 1u) & ~((1u << (unsigned)(lo - b)) - 1u);         // (hi - b <= 16)
      qsum = __builtin_amdgcn_sad_u8(v.x & byte_mask4(m & 15u), 0u, qsum);
      qsum = __builtin_amdgcn_sad_u8(v.y & byte_mask4((m >> 4) & 15u), 0u, qsum);
      qsum = __builtin_amdgcn_sad_u8(v.z & byte_mask4((m >> 8) & 15u), 0u, qsum);
      qsum = __builtin_amdgcn_sad_u8(v.w & byte_mask4((m >> 12) & 15u), 0u, qsum);
    } else {
      for (unsigned long long a = lo; a < hi; ++a) qsum += p.d[a - col_lo];            // (the stream's border granule: < 16 bytes)
    }
  }
#pragma unroll
  for (int w = kFactLanes / 2; w >= 1; w >>= 1) qsum += (uint32_t)__shfl_xor((int)qsum, w, kFactLanes);
  if (sub != 0) return;
  const long long nm = find_nm(r + 4 + body, r + 4 + bs);
  p.gene[i] = (uint32_t)g;
  if (nm > kMaxField16) {
    atomicMin(p.bad, ((unsigned long long)i << 8) | kFactSize);
    p.rec[i] = make_uint2(0u, 0u);
    return;
  }
  // ---- [EXT] pysam query_alignment_start / _end, as pack_records walks them -----------------------------------------------------
  const uint8_t* cg = r + 36 + lrn;
  const long long nc = n_cig;
  long long qs = 0;
  for (long long k = 0; k < nc; ++k) {
    const uint32_t w = rd32(cg + 4 * k), op = w & 15u;
    if (op == 5u) continue;
    if (op == 4u) qs += w >> 4; else break;
  }
  long long qe = l;
  for (long long k = nc - 1; k >= 1; --k) {
    const uint32_t w = rd32(cg + 4 * k), op = w & 15u;
    if (op == 5u) continue;
    if (op == 4u) qe -= w >> 4; else break;
  }
  long long al = qe - qs > 0 ? qe - qs : 0;
  if (al > (long long)l) al = l;
  const bool no_qual = l > 0 && p.d[q0] == 0xFFu;
  const uint32_t flags = (l == 0 ? kNoSeq : 0u) | (nm < 0 ? kNoNm : 0u) | (no_qual ? kNoQual : 0u);
  const uint32_t nm_u = (uint32_t)(nm < 0 ? 0 : nm);
  const uint32_t qmean = l > 0 ? qsum / l : 0u;
  p.rec[i] = make_uint2((uint32_t)al | (l << 11) | (flags << 22), nm_u | (qmean << 16) | (((w3 >> 8) & 0xFFu) << 24));
}

// first sorted position of every gene: begin[g] = lowest i with key[i] >= g; begin[n_genes] = n
__global__ __launch_bounds__(256) void genes_bounds_kernel(const uint32_t* key, long long n, long long n_genes, long long* begin) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  const long long prev = i == 0 ? -1 : (long long)key[i - 1];
  const long long cur = i == n ? n_genes : (long long)key[i];
  for (long long g = prev + 1; g <= cur; ++g) begin[g] = i;
}

struct SumKParams {
  const double* term;            // [n] gene order, BAM order inside a gene
  const long long* begin;        // [n_genes + 1]
  long long* aligned;            // [n_genes]
  long long* mapped;
  double* depth;
  unsigned int* heavy_count;
  unsigned int* heavy;           // [n_genes] genes left to the wave kernel
  long long n_genes;
};

__global__ __launch_bounds__(256) void genes_sum_kernel(SumKParams p) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= p.n_genes) return;
  const long long lo = p.begin[g], hi = p.begin[g + 1];
  p.aligned[g] = hi - lo;
  if (hi - lo > kHeavyGene) {
    p.heavy[atomicAdd(p.heavy_count, 1u)] = (unsigned int)g;
    return;
  }
  long long mapped = 0;
  double depth = 0.0;
  for (long long i = lo; i < hi; ++i) {
    const double t = p.term[i];
    mapped += t > 0.0;
    depth += t;
  }
  p.mapped[g] = mapped;
  p.depth[g] = depth;
}

// One wave per heavy gene: 512 terms are fetched at once (coalesced, eight loads in flight per lane) and parked in LDS;
// then every lane alike reads them back in order (same address in all lanes: a broadcast, two terms per ds_read_b128)
// and adds them one after the other, so the sequence of additions is the thread-per-gene one while the memory latency
// is paid once per 512 terms instead of once per term.
__global__ __launch_bounds__(64) void genes_sum_heavy_kernel(SumKParams p) {
  constexpr int kBatch = 8;
  __shared__ __attribute__((aligned(16))) double buf[64 * kBatch];
  if (blockIdx.x >= *p.heavy_count) return;
  const long long g = p.heavy[blockIdx.x];
  const long long lo = p.begin[g], hi = p.begin[g + 1];
  const int lane = threadIdx.x;
  long long mapped = 0;
  double depth = 0.0;
  for (long long base = lo; base < hi; base += 64 * kBatch) {
    double t[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const long long i = base + j * 64 + lane;
      t[j] = i < hi ? p.term[i] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      mapped += __popcll(__ballot(t[j] > 0.0));
      buf[j * 64 + lane] = t[j];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const long long left = hi - base;
    const int n = left < 64 * kBatch ? (int)left : 64 * kBatch;
    const double2* pairs = reinterpret_cast<const double2*>(buf);
    int k = 0;
    for (; k + 8 <= n; k += 8) {       // (terms past the end of the gene are +0.0, but stay out of the sum anyway)
      const double2 a = pairs[k / 2], b = pairs[k / 2 + 1], c = pairs[k / 2 + 2], d = pairs[k / 2 + 3];
      depth += a.x; depth += a.y; depth += b.x; depth += b.y;
      depth += c.x; depth += c.y; depth += d.x; depth += d.y;
    }
    for (; k < n; ++k) depth += buf[k];
    __builtin_amdgcn_wave_barrier();    // the next batch overwrites buf
  }
  if (lane == 0) {
    p.mapped[g] = mapped;
    p.depth[g] = depth;
  }
}

int32_t gfail(midas_snps_ctx* ctx, int32_t st, const char* msg) {
  ctx->set_error(msg);
  return st;
}

template <class F>
void host_ranges(int64_t n, F&& fn) {
  int nt = std::min(midas::cpu_budget(), 64);
  if (n < (int64_t)1 << 15) nt = 1;
  if (nt == 1) { fn((int64_t)0, n); return; }
  std::vector<std::thread> th;
  const int64_t per = (n + nt - 1) / nt;
  for (int t = 0; t < nt; ++t) {
    const int64_t lo = t * per, hi = std::min(n, lo + per);
    if (lo >= hi) break;
    th.emplace_back([&fn, lo, hi] { fn(lo, hi); });
  }
  for (auto& x : th) x.join();
}

}  // namespace
}  // namespace midas

using namespace midas;

namespace {

// The device buffers of one call; freed when it goes out of scope.
struct DevBufs {
  std::vector<void*> ptrs;
  ~DevBufs() { for (void* q : ptrs) (void)hipFree(q); }
  template <class T> hipError_t get(T** out, size_t bytes) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes ? bytes : 16);
    if (e == hipSuccess) ptrs.push_back(q);
    *out = static_cast<T*>(q);
    return e;
  }
};

#define G_TRY(call)                                                                                              \
  do {                                                                                                           \
    hipError_t e__ = (call);                                                                                     \
    if (e__ != hipSuccess) {                                                                                     \
      char buf__[384];                                                                                           \
      snprintf(buf__, sizeof buf__, "%s: %s", #call, hipGetErrorString(e__));                                    \
      (void)hipGetLastError();                                                                                   \
      return gfail(ctx, e__ == hipErrorOutOfMemory ? MIDAS_SNPS_ERR_OUT_OF_MEMORY : MIDAS_SNPS_ERR_HIP, buf__);  \
    }                                                                                                            \
  } while (0)

// The first read in BAM order that no record can be made of: the status and message of both routes (pack_records on the host,
// genes_facts_kernel / bam_genes_facts_kernel on the device; ref_id: not looked at for the latter's kinds).
int32_t raise_malformed(midas_snps_ctx* ctx, int64_t first, uint32_t kind, const int32_t* ref_id) {
  ctx->err_read = first;
  char buf[200];
  if (kind == kFactRef) {
    snprintf(buf, sizeof buf, "read %lld: reference id %lld is not a gene of the pangenome (the reference fails in getrname / genes[...])",
             (long long)first, (long long)ref_id[first]);
    return gfail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, buf);
  }
  if (kind == kFactRecord) {
    snprintf(buf, sizeof buf, "read %lld: the alignment record overruns its block_size or names no reference of the header", (long long)first);
    return gfail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, buf);
  }
  if (kind == kFactLayout) return gfail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, "negative size or CSR offsets shorter than l_seq");
  return gfail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "l_seq > 1024 or NM > 65534 is not supported");
}

// host: per read, the numbers keep_read looks at (all cores).  0, or the status of the first malformed read in BAM order.
int32_t pack_records(midas_snps_ctx* ctx, const midas_snps_reads* reads, const int32_t* ref_id, int64_t n_genes, std::vector<uint2>* recs,
                     int32_t* max_l_out) {
  const int64_t n = reads->n_reads;
  recs->resize((size_t)n);
  std::atomic<int64_t> bad_ref{INT64_MAX}, bad_layout{INT64_MAX}, bad_size{INT64_MAX};
  std::atomic<int32_t> max_l_all{0};
  auto lower = [](std::atomic<int64_t>& a, int64_t v) {
    int64_t cur = a.load();
    while (v < cur && !a.compare_exchange_weak(cur, v)) {}
  };
  host_ranges(n, [&](int64_t lo, int64_t hi) {
    int32_t max_l = 0;
    for (int64_t i = lo; i < hi; ++i) {
      const int64_t g = ref_id[i];
      if (g < 0 || g >= n_genes) { lower(bad_ref, i); continue; }
      const int64_t l = reads->l_seq[i];
      const int64_t nc = reads->cigar_off[i + 1] - reads->cigar_off[i];
      if (l < 0 || nc < 0 || reads->qual_off[i + 1] - reads->qual_off[i] < l) { lower(bad_layout, i); continue; }
      if (l > kMaxLSeq || reads->nm[i] > kMaxField16) { lower(bad_size, i); continue; }
      const uint32_t* cg = reads->cigar + reads->cigar_off[i];
      // [EXT] pysam query_alignment_start / _end: leading S run (hopping over H); trailing S run found by a backward
      // walk over ops n-1 .. 1 (op 0 is never inspected)
      int64_t qs = 0;
      for (int64_t k = 0; k < nc; ++k) {
        const uint32_t op = cg[k] & 15u;
        if (op == 5u) continue;
        if (op == 4u) qs += cg[k] >> 4; else break;
      }
      int64_t qe = l;
      for (int64_t k = nc - 1; k >= 1; --k) {
        const uint32_t op = cg[k] & 15u;
        if (op == 5u) continue;
        if (op == 4u) qe -= cg[k] >> 4; else break;
      }
      int64_t al = qe - qs > 0 ? qe - qs : 0;
      if (al > l) al = l;                       // (clips shorter than the read: cannot exceed it)
      const uint8_t* q = reads->qual + reads->qual_off[i];
      uint32_t qsum = 0;
      for (int64_t x = 0; x < l; ++x) qsum += q[x];
      const uint32_t flags = (l == 0 ? kNoSeq : 0u) | (reads->nm[i] < 0 ? kNoNm : 0u) | ((l > 0 && q[0] == 0xFF) ? kNoQual : 0u);
      const uint32_t nm = (uint32_t)(reads->nm[i] < 0 ? 0 : reads->nm[i]);
      const uint32_t qmean = l > 0 ? qsum / (uint32_t)l : 0u;
      (*recs)[(size_t)i] = make_uint2((uint32_t)al | ((uint32_t)l << 11) | (flags << 22), nm | (qmean << 16) | ((uint32_t)reads->mapq[i] << 24));
      max_l = std::max<int32_t>(max_l, (int32_t)l);
    }
    int32_t cur = max_l_all.load();
    while (max_l > cur && !max_l_all.compare_exchange_weak(cur, max_l)) {}
  });
  *max_l_out = max_l_all.load();
  // the first malformed read in BAM order decides, as a single forward pass would
  const int64_t first = std::min(bad_ref.load(), std::min(bad_layout.load(), bad_size.load()));
  if (first == INT64_MAX) return MIDAS_SNPS_OK;
  return raise_malformed(ctx, first, first == bad_ref.load() ? kFactRef : first == bad_layout.load() ? kFactLayout : kFactSize, ref_id);
}

int32_t raise_status(midas_snps_ctx* ctx, unsigned long long err) {
  const int32_t kind = (int32_t)(err & 0xFF);
  ctx->err_read = (int64_t)(err >> 8);
  char buf[200];
  snprintf(buf, sizeof buf, "read %lld: keep_read would raise (%s)", (long long)ctx->err_read,
           kind == 1 ? "no SEQ: TypeError" : kind == 2 ? "no NM tag: KeyError" : kind == 3 ? "aligned length 0: ZeroDivisionError"
                                                                                              : "no QUAL: TypeError");
  ctx->set_error(buf);
  return kind;
}

// The device buffers behind the records, whoever made them and wherever they were allocated: (gene, record) pairs in, per-gene
// numbers out.
struct GenesBufs {
  uint2* recs; uint32_t* key; uint32_t* key_b; double* term; double* term_b; int64_t* len; FilterTables* ft;
  long long* begin; long long* al; long long* mp; double* dp; unsigned long long* err; unsigned int* heavy; uint32_t* hist;
};

// The tail every route shares: filter (filter: the terms are made from b.recs; else b.term holds them), the terms handed back
// (out_term), and with out_aligned the stable sort by gene, the bounds, the ordered sums and their way down.  Everything is queued
// on s and nothing is waited for; e1 is recorded behind the last kernel.
int32_t genes_tail(midas_snps_ctx* ctx, hipStream_t s, const midas_snps_thresholds* thr, const GenesBufs& b, int64_t n, int64_t n_genes, bool filter,
                   double* out_term, int64_t* out_aligned, int64_t* out_mapped, double* out_depth, hipEvent_t e1) {
  const bool sums = out_aligned != nullptr;
  int key_bits = 1;
  while (key_bits < 32 && ((int64_t)1 << key_bits) < n_genes) ++key_bits;
  if (filter && n > 0) {
    FilterKParams f;
    f.rec = b.recs; f.gene = b.key; f.gene_len = b.len; f.filt = b.ft; f.term = b.term; f.err = b.err; f.n = n;
    f.mapq = thr->mapq; f.readq = thr->readq;
    hipLaunchKernelGGL(genes_filter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, f);
    G_TRY(hipGetLastError());
  }
  if (out_term && n > 0) G_TRY(hipMemcpyAsync(out_term, b.term, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  if (sums && n_genes > 0) {
    uint32_t* d_key_sorted = b.key;
    double* d_term_sorted = b.term;
    G_TRY(launch_sort_pairs_f64(b.key, b.term, b.key_b, b.term_b, n, key_bits, b.hist, s, &d_key_sorted, &d_term_sorted));
    hipLaunchKernelGGL(genes_bounds_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s, d_key_sorted, (long long)n,
                       (long long)n_genes, b.begin);
    G_TRY(hipGetLastError());
    SumKParams k;
    k.term = d_term_sorted; k.begin = b.begin; k.aligned = b.al; k.mapped = b.mp; k.depth = b.dp;
    k.heavy_count = b.heavy; k.heavy = b.heavy + 1; k.n_genes = n_genes;
    hipLaunchKernelGGL(genes_sum_kernel, dim3((unsigned)((n_genes + 255) / 256)), dim3(256), 0, s, k);
    G_TRY(hipGetLastError());
    // at most n / kHeavyGene genes are heavy; idle waves leave at once
    const long long max_heavy = std::min<long long>(n_genes, n / kHeavyGene);
    if (max_heavy > 0) {
      hipLaunchKernelGGL(genes_sum_heavy_kernel, dim3((unsigned)max_heavy), dim3(64), 0, s, k);
      G_TRY(hipGetLastError());
    }
    G_TRY(hipEventRecord(e1, s));
    G_TRY(hipMemcpyAsync(out_aligned, b.al, (size_t)n_genes * 8, hipMemcpyDeviceToHost, s));
    G_TRY(hipMemcpyAsync(out_mapped, b.mp, (size_t)n_genes * 8, hipMemcpyDeviceToHost, s));
    G_TRY(hipMemcpyAsync(out_depth, b.dp, (size_t)n_genes * 8, hipMemcpyDeviceToHost, s));
  } else {
    G_TRY(hipEventRecord(e1, s));
  }
  return MIDAS_SNPS_OK;
}

// One call, either half or both.  reads != nullptr: the terms are made here (records + filter kernel) from the reads and
// their genes `gene` (= ref_id) -- the records by the host's cores (pack_records), or, with payload_on_device (reads->qual /
// ->cigar are device addresses), by genes_facts_kernel; everything behind the records is the same; else `term_in` holds them.  out_term != nullptr: they are handed back (and, with no sums asked
// for, that is all).  out_aligned != nullptr: sort + bounds + sums.
int32_t genes_run(midas_snps_ctx* ctx, const midas_snps_thresholds* thr, const midas_snps_reads* reads, int64_t n, const int32_t* gene,
                  const double* term_in, int64_t n_genes, const int64_t* gene_length, double* out_term, int64_t* out_aligned,
                  int64_t* out_mapped, double* out_depth, float* out_kernel_ms, bool payload_on_device = false) {
  ctx->clear_error();
  ctx->err_read = -1;
  if (out_kernel_ms) *out_kernel_ms = 0.f;
  if (n > 0x7FFFFFFFll || n_genes > 0x7FFFFFFFll) return gfail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "more than 2^31-1 reads or genes");
  const bool filter = reads != nullptr, sums = out_aligned != nullptr;
  std::vector<uint2> recs;
  FilterTables ft;
  memset(&ft, 0, sizeof ft);
  const bool facts = filter && payload_on_device;
  if (facts) {
    // (no pass over the reads here: the tables for every length a record can hold -- an entry is only ever read at a read's own
    // lengths, so the ones pack_records' max_l would have left zero are never looked at)
    build_filter_tables(thr->mapid, thr->aln_cov, kMaxLSeq, &ft);
  } else if (filter) {
    int32_t max_l = 0;
    const int32_t st = pack_records(ctx, reads, gene, n_genes, &recs, &max_l);
    if (st != MIDAS_SNPS_OK) return st;
    build_filter_tables(thr->mapid, thr->aln_cov, max_l, &ft);
  } else {
    for (int64_t i = 0; i < n; ++i)
      if (gene[i] < 0 || gene[i] >= n_genes) {
        ctx->err_read = i;
        return gfail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, "a pair's gene index is outside the gene table");
      }
  }
  // ---- device ------------------------------------------------------------------------------------------------------
  DevBufs dev;
  G_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t ng = (size_t)(n_genes > 0 ? n_genes : 1), nr = (size_t)(n > 0 ? n : 1);
  uint2* d_recs = nullptr; uint32_t* d_key = nullptr; uint32_t* d_key_b = nullptr; double* d_term = nullptr; double* d_term_b = nullptr;
  int64_t* d_len = nullptr; FilterTables* d_ft = nullptr; long long* d_begin = nullptr; long long* d_al = nullptr; long long* d_mp = nullptr;
  double* d_dp = nullptr; unsigned long long* d_err = nullptr; unsigned int* d_heavy = nullptr; uint32_t* d_hist = nullptr;
  int32_t* d_lseq = nullptr; int32_t* d_nm = nullptr; uint8_t* d_mapq = nullptr; long long* d_qoff = nullptr; long long* d_coff = nullptr;
  G_TRY(dev.get(&d_key, nr * 4));
  G_TRY(dev.get(&d_term, nr * 8));
  G_TRY(dev.get(&d_err, 16));
  if (filter) {
    G_TRY(dev.get(&d_recs, nr * sizeof(uint2)));
    G_TRY(dev.get(&d_len, ng * 8));
    G_TRY(dev.get(&d_ft, sizeof(FilterTables)));
  }
  if (facts) {        // the small columns of the reads: 29 bytes a read, uploaded once
    G_TRY(dev.get(&d_lseq, nr * 4));
    G_TRY(dev.get(&d_nm, nr * 4));
    G_TRY(dev.get(&d_mapq, nr));
    G_TRY(dev.get(&d_qoff, (nr + 1) * 8));
    G_TRY(dev.get(&d_coff, (nr + 1) * 8));
  }
  if (sums) {
    G_TRY(dev.get(&d_key_b, nr * 4));
    G_TRY(dev.get(&d_term_b, nr * 8));
    G_TRY(dev.get(&d_hist, sort_scratch_words((long long)nr) * 4));
    G_TRY(dev.get(&d_begin, (ng + 1) * 8));
    G_TRY(dev.get(&d_al, ng * 8));
    G_TRY(dev.get(&d_mp, ng * 8));
    G_TRY(dev.get(&d_dp, ng * 8));
    G_TRY(dev.get(&d_heavy, (ng + 1) * 4));
  }
  if (n > 0) {
    G_TRY(hipMemcpyAsync(d_key, gene, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (facts) {
      G_TRY(hipMemcpyAsync(d_lseq, reads->l_seq, (size_t)n * 4, hipMemcpyHostToDevice, s));
      G_TRY(hipMemcpyAsync(d_nm, reads->nm, (size_t)n * 4, hipMemcpyHostToDevice, s));
      G_TRY(hipMemcpyAsync(d_mapq, reads->mapq, (size_t)n, hipMemcpyHostToDevice, s));
      G_TRY(hipMemcpyAsync(d_qoff, reads->qual_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
      G_TRY(hipMemcpyAsync(d_coff, reads->cigar_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    } else if (filter) G_TRY(hipMemcpyAsync(d_recs, recs.data(), (size_t)n * sizeof(uint2), hipMemcpyHostToDevice, s));
    else G_TRY(hipMemcpyAsync(d_term, term_in, (size_t)n * 8, hipMemcpyHostToDevice, s));
  }
  if (filter) {
    if (n_genes > 0) G_TRY(hipMemcpyAsync(d_len, gene_length, (size_t)n_genes * 8, hipMemcpyHostToDevice, s));
    G_TRY(hipMemcpyAsync(d_ft, &ft, sizeof ft, hipMemcpyHostToDevice, s));
  }
  G_TRY(hipMemsetAsync(d_err, 0xFF, 16, s));        // [0]: the filter's, [1]: the facts kernel's
  if (sums) G_TRY(hipMemsetAsync(d_heavy, 0, 4, s));
  struct EvGuard {      // (constructed before either event exists: a failing second create must not leak the first)
    hipEvent_t a = nullptr, b = nullptr, c = nullptr;
    ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); if (c) (void)hipEventDestroy(c); }
  } evg;
  G_TRY(hipEventCreate(&evg.a));
  G_TRY(hipEventCreate(&evg.b));
  if (facts) G_TRY(hipEventCreate(&evg.c));
  const hipEvent_t e0 = evg.a, e1 = evg.b, ef = evg.c;
  unsigned long long err[2] = {~0ull, ~0ull};
  G_TRY(hipEventRecord(e0, s));
  if (facts) {
    if (n > 0) {
      // (qual_off[n] / cigar_off[n]: the columns' sizes -- what the caller says lies at reads->qual / ->cigar)
      FactsKParams f;
      f.l_seq = d_lseq; f.nm = d_nm; f.mapq = d_mapq; f.qual_off = d_qoff; f.cigar_off = d_coff;
      f.qual = reads->qual; f.cigar = reads->cigar; f.qual_total = reads->qual_off[n]; f.cigar_total = reads->cigar_off[n];
      f.gene = d_key; f.rec = d_recs; f.bad = d_err + 1; f.n = n; f.n_genes = n_genes;
      constexpr int kPerBlock = 256 / kFactLanes;
      hipLaunchKernelGGL(genes_facts_kernel, dim3((unsigned)((n + kPerBlock - 1) / kPerBlock)), dim3(256), 0, s, f);
      G_TRY(hipGetLastError());
    }
    G_TRY(hipEventRecord(ef, s));
  }
  GenesBufs gb;
  gb.recs = d_recs; gb.key = d_key; gb.key_b = d_key_b; gb.term = d_term; gb.term_b = d_term_b; gb.len = d_len; gb.ft = d_ft;
  gb.begin = d_begin; gb.al = d_al; gb.mp = d_mp; gb.dp = d_dp; gb.err = d_err; gb.heavy = d_heavy; gb.hist = d_hist;
  const int32_t tst = genes_tail(ctx, s, thr, gb, n, n_genes, filter, out_term, out_aligned, out_mapped, out_depth, e1);
  if (tst != MIDAS_SNPS_OK) return tst;
  G_TRY(hipMemcpyAsync(err, d_err, 16, hipMemcpyDeviceToHost, s));
  G_TRY(hipStreamSynchronize(s));
  float ms = 0.f;
  G_TRY(hipEventElapsedTime(&ms, e0, e1));
  if (out_kernel_ms) *out_kernel_ms = ms;
  if (facts) {
    float ms_f = 0.f;
    G_TRY(hipEventElapsedTime(&ms_f, e0, ef));
    ctx->genes_ms[0] = ms_f;
    ctx->genes_ms[1] = ms - ms_f;
  }
  // a read no record could be made of comes first, as pack_records returns before the filter has seen anything
  if (err[1] != ~0ull) return raise_malformed(ctx, (int64_t)(err[1] >> 8), (uint32_t)(err[1] & 0xFF), gene);
  if (err[0] != ~0ull) return raise_status(ctx, err[0]);
  return MIDAS_SNPS_OK;
}

bool reads_ok(const midas_snps_reads* reads, const int32_t* ref_id) {
  return reads && reads->n_reads >= 0 &&
         (reads->n_reads == 0 || (ref_id && reads->mapq && reads->nm && reads->l_seq && reads->qual_off && reads->cigar_off && reads->qual && reads->cigar));
}

}  // namespace

// midas_genes_count_bam behind its decode (bam_device.hip): the facts from the records where they lie, then the tail.
int32_t midas_ctx::genes_count_stream(midas_snps_ctx* ctx, const uint8_t* d, unsigned long long total, const unsigned long long* rec_off, long long n,
                                      uint8_t* scratch, size_t scratch_bytes, GenesBamCall* call) {
  ctx->clear_error();
  ctx->err_read = -1;
  const int64_t n_genes = call->n_genes;
  if (n > 0x7FFFFFFFll || n_genes > 0x7FFFFFFFll) return gfail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "more than 2^31-1 reads or genes");
  FilterTables ft;
  memset(&ft, 0, sizeof ft);
  build_filter_tables(call->thr->mapid, call->thr->aln_cov, kMaxLSeq, &ft);        // (every length a record can hold, as midas_genes_count_device)
  hipStream_t s = ctx->stream;
  const size_t ng = (size_t)(n_genes > 0 ? n_genes : 1), nr = (size_t)(n > 0 ? n : 1);
  size_t at = 0;
  bool fits = true;
  auto take = [&](size_t bytes) -> void* {       // pieces of the caller's scratch, 256-byte aligned
    uint8_t* q = scratch + at;
    at += (bytes + 255) & ~(size_t)255;
    if (at > scratch_bytes) fits = false;
    return q;
  };
  GenesBufs b;
  b.key = static_cast<uint32_t*>(take(nr * 4)); b.term = static_cast<double*>(take(nr * 8)); b.err = static_cast<unsigned long long*>(take(16));
  b.recs = static_cast<uint2*>(take(nr * sizeof(uint2))); b.len = static_cast<int64_t*>(take(ng * 8)); b.ft = static_cast<FilterTables*>(take(sizeof(FilterTables)));
  b.key_b = static_cast<uint32_t*>(take(nr * 4)); b.term_b = static_cast<double*>(take(nr * 8));
  b.hist = static_cast<uint32_t*>(take(sort_scratch_words((long long)nr) * 4));
  b.begin = static_cast<long long*>(take((ng + 1) * 8)); b.al = static_cast<long long*>(take(ng * 8)); b.mp = static_cast<long long*>(take(ng * 8));
  b.dp = static_cast<double*>(take(ng * 8)); b.heavy = static_cast<unsigned int*>(take((ng + 1) * 4));
  if (!fits) return gfail(ctx, MIDAS_SNPS_ERR_OUT_OF_MEMORY, "genes count over a BAM: the decode's arena is too small for the per-read terms");
  if (n_genes > 0) G_TRY(hipMemcpyAsync(b.len, call->gene_length, (size_t)n_genes * 8, hipMemcpyHostToDevice, s));
  G_TRY(hipMemcpyAsync(b.ft, &ft, sizeof ft, hipMemcpyHostToDevice, s));
  G_TRY(hipMemsetAsync(b.err, 0xFF, 16, s));          // [0]: the filter's, [1]: the facts kernel's
  G_TRY(hipMemsetAsync(b.heavy, 0, 4, s));
  if (n > 0) {
    BamFactsKParams f;
    f.d = d; f.total = total; f.rec_off = rec_off; f.gene = b.key; f.rec = b.recs; f.bad = b.err + 1; f.n = n; f.n_genes = n_genes;
    constexpr int kPerBlock = 256 / kFactLanes;
    hipLaunchKernelGGL(bam_genes_facts_kernel, dim3((unsigned)((n + kPerBlock - 1) / kPerBlock)), dim3(256), 0, s, f);
    G_TRY(hipGetLastError());
  }
  G_TRY(hipEventRecord(call->ev[3], s));
  int64_t dummy_a = 0, dummy_m = 0;
  double dummy_d = 0.0;
  const int32_t tst = genes_tail(ctx, s, call->thr, b, n, n_genes, true, nullptr, n_genes > 0 ? call->out_aligned : &dummy_a,
                                 n_genes > 0 ? call->out_mapped : &dummy_m, n_genes > 0 ? call->out_depth : &dummy_d, call->ev[4]);
  if (tst != MIDAS_SNPS_OK) return tst;
  unsigned long long err[2] = {~0ull, ~0ull};
  G_TRY(hipMemcpyAsync(err, b.err, 16, hipMemcpyDeviceToHost, s));
  G_TRY(hipEventRecord(call->ev[5], s));
  G_TRY(hipStreamSynchronize(s));
  for (int k = 1; k < 6; ++k) G_TRY(hipEventElapsedTime(&call->ms[k], call->ev[k - 1], call->ev[k]));
  // a read no record could be made of comes first, as on the host's route
  if (err[1] != ~0ull) return raise_malformed(ctx, (int64_t)(err[1] >> 8), (uint32_t)(err[1] & 0xFF), nullptr);
  if (err[0] != ~0ull) return raise_status(ctx, err[0]);
  return MIDAS_SNPS_OK;
}

extern "C" int32_t midas_genes_count(midas_snps_ctx* ctx, const midas_snps_thresholds* thr, const midas_snps_reads* reads,
                                     const int32_t* ref_id, int64_t n_genes, const int64_t* gene_length,
                                     int64_t* out_aligned, int64_t* out_mapped, double* out_depth, float* out_kernel_ms) {
  if (!ctx || !thr || n_genes < 0 || !reads_ok(reads, ref_id) || (n_genes > 0 && (!gene_length || !out_aligned || !out_mapped || !out_depth)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  int64_t dummy_a = 0, dummy_m = 0;
  double dummy_d = 0.0;
  return genes_run(ctx, thr, reads, reads->n_reads, ref_id, nullptr, n_genes, gene_length, nullptr, n_genes > 0 ? out_aligned : &dummy_a,
                   n_genes > 0 ? out_mapped : &dummy_m, n_genes > 0 ? out_depth : &dummy_d, out_kernel_ms);
}

extern "C" int32_t midas_genes_count_device(midas_snps_ctx* ctx, const midas_snps_thresholds* thr, const midas_snps_reads* reads,
                                            const int32_t* ref_id, int64_t n_genes, const int64_t* gene_length,
                                            int64_t* out_aligned, int64_t* out_mapped, double* out_depth, float* out_kernel_ms) {
  if (!ctx || !thr || n_genes < 0 || !reads_ok(reads, ref_id) || (n_genes > 0 && (!gene_length || !out_aligned || !out_mapped || !out_depth)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  if (reads->n_reads > 0 && (reads->qual_off[reads->n_reads] < 0 || reads->cigar_off[reads->n_reads] < 0)) return MIDAS_SNPS_ERR_INVALID_ARG;
  int64_t dummy_a = 0, dummy_m = 0;
  double dummy_d = 0.0;
  return genes_run(ctx, thr, reads, reads->n_reads, ref_id, nullptr, n_genes, gene_length, nullptr, n_genes > 0 ? out_aligned : &dummy_a,
                   n_genes > 0 ? out_mapped : &dummy_m, n_genes > 0 ? out_depth : &dummy_d, out_kernel_ms, true);
}

extern "C" int32_t midas_genes_count_timing(const midas_snps_ctx* ctx, float* out_ms2) {
  if (!ctx || !out_ms2) return MIDAS_SNPS_ERR_INVALID_ARG;
  out_ms2[0] = ctx->genes_ms[0];
  out_ms2[1] = ctx->genes_ms[1];
  return MIDAS_SNPS_OK;
}

extern "C" int32_t midas_genes_terms(midas_snps_ctx* ctx, const midas_snps_thresholds* thr, const midas_snps_reads* reads,
                                     const int32_t* ref_id, int64_t n_genes, const int64_t* gene_length, double* out_term,
                                     float* out_kernel_ms) {
  if (!ctx || !thr || n_genes < 0 || !reads_ok(reads, ref_id) || (n_genes > 0 && !gene_length) || (reads->n_reads > 0 && !out_term))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  return genes_run(ctx, thr, reads, reads->n_reads, ref_id, nullptr, n_genes, gene_length, out_term, nullptr, nullptr, nullptr, out_kernel_ms);
}

extern "C" int32_t midas_genes_sum(midas_snps_ctx* ctx, int64_t n_pairs, const int32_t* gene, const double* term, int64_t n_genes,
                                   int64_t* out_aligned, int64_t* out_mapped, double* out_depth, float* out_kernel_ms) {
  if (!ctx || n_pairs < 0 || n_genes < 0 || (n_pairs > 0 && (!gene || !term)) || (n_genes > 0 && (!out_aligned || !out_mapped || !out_depth)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  int64_t dummy_a = 0, dummy_m = 0;
  double dummy_d = 0.0;
  return genes_run(ctx, nullptr, nullptr, n_pairs, gene, term, n_genes, nullptr, nullptr, n_genes > 0 ? out_aligned : &dummy_a,
                   n_genes > 0 ? out_mapped : &dummy_m, n_genes > 0 ? out_depth : &dummy_d, out_kernel_ms);
}
