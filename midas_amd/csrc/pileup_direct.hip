// gfx950 (CDNA4) pileup kernel of the MIDAS SNP path that reads the reads in input order: per read ONE 16-byte record (pos,
// l_seq, n_cigar, NM, mapq, payload offset -- layout.h DirectRec) and its payload -- BAM's CIGAR, the sum of its qualities and
// ONE byte a base (layout.h dense_byte) -- one run per read: nothing sorted or decided beforehand, ONE visit per read.
// Integer counting: no MFMA.
//
// Reference semantics implemented here (citations into /root/reference):
//   keep_read                       midas/run/snps.py:141-162  (query_alignment_sequence :145, np.mean(query_qualities) :151)
//   count_coverage call site        midas/run/snps.py:194-199  ([EXT] pysam: get_aligned_pairs(matches_only), qual >= quality_threshold,
//                                   only 'A','C','G','T' counted)
//   depth / covered / total_depth   midas/run/snps.py:204-213
//   str(rec.seq).upper()            midas/run/snps.py:62
// The reference filters and counts a read in one pass (keep_read inside count_coverage's iterator); so does this kernel.
//
// Work decomposition: as in pileup_tiles.hip -- tiles of <= 2048 sites, a persistent 256-thread workgroup per item (four per CU), tallies
// in LDS as [site][A,C,G,T] u32, one coalesced write-out per tile, items handed out by per-XCD counters.
//
// Stream.  The ranges pass (index_direct.hip, 4 bytes per read) left, per tile, the run [tbegin, tend) of read indices that
// can touch the tile -- the input is position-sorted, so that is a contiguous run of the read arrays.  It is dealt to the
// workgroup's waves as wave-iterations of floor(64 / lanes per read) reads.
//
// Lane mapping.  A lane owns LB (30, 32 or 38: direct_lane_bases below) consecutive bases of a read's STORED query: two 16-byte
// loads of base bytes, and an 8-byte one for 38.  A read of l_seq bases takes ceil(l_seq / LB) adjacent lanes (4 for 150 bp, 5
// for 151).  A lane's loads are issued two iterations (the payload offset and lengths of its read, out of the read's record) and
// one iteration (its bases, off ONE scalar base per wave-iteration -- the payload of the iteration's first read -- plus a
// 32-bit lane offset) ahead of their use; none of them sits in a branch.
//
// Per read, ONCE per read.  What does not depend on the lane -- the shape of the read's CIGAR, ONE or TWO gap-free match runs
// (direct_common.h ReadShape: clips, at most one insertion / deletion / skip -- what an aligner writes for nearly every read), the
// two filter tables, keep_read, the read's count and its error -- is done by ONE lane per read for a PHASE of up to four of the
// wave's iterations (64 reads: one per lane) from loads of its own (record, first four CIGAR ops, quality sum: once per read), and
// handed to the lanes that hold the read's bases in four words: a DPP quad move where a read has four lanes, ds_bpermute_b32
// otherwise.  Those lanes clip the runs to the tile and tally them straight from the shape, the lane that holds the indel in a
// second masked pass.  Anything else (several indels, pads, odd clips, no NM / SEQ, a start off the contig) is walked op by op
// by the lanes of the read at the start of its phase, the slow path, from loads of its own.
//
// Per base: the counter offsets of four bases are `(word << 2) & 0x0C0C0C0C` (two ALU ops a word); then per base one SDWA OR
// forming the LDS address, one SDWA compare `byte >= thr` (thr = layout.h dense_threshold(baseq), wave-uniform) into a lane
// mask, one returnless ds_add under the mask.  N and the other non-A/C/G/T codes have bytes below every threshold.
// Clipping (soft clips, segment borders, tile edges, the read's tail) zeroes the bytes outside: two rows of a byte-mask
// table from LDS per group of a partial pass.
// The read's mean quality: the sum stored behind its CIGAR; sum(q) < readq * l_seq is the reference's np.mean(q) < readq exactly.
#include "direct_common.h"
#include "pileup_common.h"

#include <type_traits>

namespace midas {

using namespace dev;
using namespace pile;
using namespace direct;

namespace {

// (developer listings: hipcc -S -DMIDAS_ISA_MARKS puts `; MARK name` lines into the assembly, tools/isa/segments.py counts between them)
#ifdef MIDAS_ISA_MARKS
#define MIDAS_MARK(name) asm volatile("; MARK " name)
#else
#define MIDAS_MARK(name) do { } while (0)
#endif

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Lane J of every quad's word, on all four lanes of the quad: one DPP move, nothing through the LDS pipeline.
template <int J>
__device__ __forceinline__ uint32_t quad_take(uint32_t x) {
  static_assert(J >= 0 && J < 4, "a lane of the quad");
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, J * 0x55, 0xF, 0xF, false);
}

// DirectParams again, out of the kernel's argument segment: a field that only a tile's end or a rare branch uses is loaded where
// it is used (one scalar load) and holds no scalar registers through the stream loop, which has none to spare.  (The empty asm
// keeps the compiler from merging these loads with the ones at the kernel's top.)
typedef const __attribute__((address_space(4))) DirectParams* ParamsAgain;
__device__ __forceinline__ ParamsAgain params_again() {
  ParamsAgain k = (ParamsAgain)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}

// A scalar in a register of its own: a word of a block of scalars that one load brought (the kernel's arguments, a tile's eight
// words) otherwise keeps the whole block alive, and the block is saved and restored as one.
__device__ __forceinline__ int own_scalar(int x) {
  int y;
  asm volatile("s_mov_b32 %0, %1" : "=s"(y) : "s"(x));
  return y;
}

// Eight bases of one lane: b0 / b1 two words of four base bytes (layout.h dense_byte, bases in order), thr the byte threshold
// (dense_threshold, wave-uniform).  Per base one SDWA OR forming the LDS address of its counter ((byte & 3) << 2, two ALU ops a
// word), one SDWA compare `byte >= thr` into a lane mask, one returnless ds_add under it.
template <int OFF, int NB>
__device__ __forceinline__ void tally_group(uint32_t b0, uint32_t b1, uint32_t thr, uint32_t abase, uint32_t one) {
  static_assert(NB == 8 || NB == 6, "a group holds 8 bases, or 6 at the end of a 30- or 38-base lane");
  const uint32_t c0 = (b0 << 2) & 0x0C0C0C0Cu, c1 = (b1 << 2) & 0x0C0C0C0Cu;
  uint32_t t0, t1, t2, t3, t4, t5, t6, t7;
  unsigned long long m0, m1, m2, m3, m4, m5, m6, m7, save;
  if (NB == 8) {
    asm volatile(
        "v_or_b32_sdwa %[t0], %[ab], %[c0] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0\n\t"
        "v_or_b32_sdwa %[t1], %[ab], %[c0] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1\n\t"
        "v_or_b32_sdwa %[t2], %[ab], %[c0] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2\n\t"
        "v_or_b32_sdwa %[t3], %[ab], %[c0] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3\n\t"
        "v_or_b32_sdwa %[t4], %[ab], %[c1] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0\n\t"
        "v_or_b32_sdwa %[t5], %[ab], %[c1] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1\n\t"
        "v_or_b32_sdwa %[t6], %[ab], %[c1] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2\n\t"
        "v_or_b32_sdwa %[t7], %[ab], %[c1] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3\n\t"
        "v_cmp_ge_u32_sdwa %[m0], %[b0], %[th] src0_sel:BYTE_0 src1_sel:DWORD\n\t"
        "v_cmp_ge_u32_sdwa %[m1], %[b0], %[th] src0_sel:BYTE_1 src1_sel:DWORD\n\t"
        "v_cmp_ge_u32_sdwa %[m2], %[b0], %[th] src0_sel:BYTE_2 src1_sel:DWORD\n\t"
        "v_cmp_ge_u32_sdwa %[m3], %[b0], %[th] src0_sel:BYTE_3 src1_sel:DWORD\n\t"
        "v_cmp_ge_u32_sdwa %[m4], %[b1], %[th] src0_sel:BYTE_0 src1_sel:DWORD\n\t"
        "v_cmp_ge_u32_sdwa %[m5], %[b1], %[th] src0_sel:BYTE_1 src1_sel:DWORD\n\t"
        "v_cmp_ge_u32_sdwa %[m6], %[b1], %[th] src0_sel:BYTE_2 src1_sel:DWORD\n\t"
        "v_cmp_ge_u32_sdwa %[m7], %[b1], %[th] src0_sel:BYTE_3 src1_sel:DWORD\n\t"
        "s_mov_b64 %[sv], exec\n\t"
        "s_mov_b64 exec, %[m0]\n\t"
        "ds_add_u32 %[t0], %[one] offset:%[off]\n\t"
        "s_mov_b64 exec, %[m1]\n\t"
        "ds_add_u32 %[t1], %[one] offset:%[off]+16\n\t"
        "s_mov_b64 exec, %[m2]\n\t"
        "ds_add_u32 %[t2], %[one] offset:%[off]+32\n\t"
        "s_mov_b64 exec, %[m3]\n\t"
        "ds_add_u32 %[t3], %[one] offset:%[off]+48\n\t"
        "s_mov_b64 exec, %[m4]\n\t"
        "ds_add_u32 %[t4], %[one] offset:%[off]+64\n\t"
        "s_mov_b64 exec, %[m5]\n\t"
        "ds_add_u32 %[t5], %[one] offset:%[off]+80\n\t"
        "s_mov_b64 exec, %[m6]\n\t"
        "ds_add_u32 %[t6], %[one] offset:%[off]+96\n\t"
        "s_mov_b64 exec, %[m7]\n\t"
        "ds_add_u32 %[t7], %[one] offset:%[off]+112\n\t"
        "s_mov_b64 exec, %[sv]"
        : [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), [t4] "=&v"(t4), [t5] "=&v"(t5), [t6] "=&v"(t6),
          [t7] "=&v"(t7), [m0] "=&s"(m0), [m1] "=&s"(m1), [m2] "=&s"(m2), [m3] "=&s"(m3), [m4] "=&s"(m4), [m5] "=&s"(m5),
          [m6] "=&s"(m6), [m7] "=&s"(m7), [sv] "=&s"(save)
        : [b0] "v"(b0), [b1] "v"(b1), [th] "v"(thr), [c0] "v"(c0), [c1] "v"(c1), [ab] "v"(abase), [one] "v"(one), [off] "n"(OFF)
        : "memory");
  } else {
    asm volatile(
        "v_or_b32_sdwa %[t0], %[ab], %[c0] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0\n\t"
        "v_or_b32_sdwa %[t1], %[ab], %[c0] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1\n\t"
        "v_or_b32_sdwa %[t2], %[ab], %[c0] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2\n\t"
        "v_or_b32_sdwa %[t3], %[ab], %[c0] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3\n\t"
        "v_or_b32_sdwa %[t4], %[ab], %[c1] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0\n\t"
        "v_or_b32_sdwa %[t5], %[ab], %[c1] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1\n\t"
        "v_cmp_ge_u32_sdwa %[m0], %[b0], %[th] src0_sel:BYTE_0 src1_sel:DWORD\n\t"
        "v_cmp_ge_u32_sdwa %[m1], %[b0], %[th] src0_sel:BYTE_1 src1_sel:DWORD\n\t"
        "v_cmp_ge_u32_sdwa %[m2], %[b0], %[th] src0_sel:BYTE_2 src1_sel:DWORD\n\t"
        "v_cmp_ge_u32_sdwa %[m3], %[b0], %[th] src0_sel:BYTE_3 src1_sel:DWORD\n\t"
        "v_cmp_ge_u32_sdwa %[m4], %[b1], %[th] src0_sel:BYTE_0 src1_sel:DWORD\n\t"
        "v_cmp_ge_u32_sdwa %[m5], %[b1], %[th] src0_sel:BYTE_1 src1_sel:DWORD\n\t"
        "s_mov_b64 %[sv], exec\n\t"
        "s_mov_b64 exec, %[m0]\n\t"
        "ds_add_u32 %[t0], %[one] offset:%[off]\n\t"
        "s_mov_b64 exec, %[m1]\n\t"
        "ds_add_u32 %[t1], %[one] offset:%[off]+16\n\t"
        "s_mov_b64 exec, %[m2]\n\t"
        "ds_add_u32 %[t2], %[one] offset:%[off]+32\n\t"
        "s_mov_b64 exec, %[m3]\n\t"
        "ds_add_u32 %[t3], %[one] offset:%[off]+48\n\t"
        "s_mov_b64 exec, %[m4]\n\t"
        "ds_add_u32 %[t4], %[one] offset:%[off]+64\n\t"
        "s_mov_b64 exec, %[m5]\n\t"
        "ds_add_u32 %[t5], %[one] offset:%[off]+80\n\t"
        "s_mov_b64 exec, %[sv]"
        : [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), [t4] "=&v"(t4), [t5] "=&v"(t5), [m0] "=&s"(m0),
          [m1] "=&s"(m1), [m2] "=&s"(m2), [m3] "=&s"(m3), [m4] "=&s"(m4), [m5] "=&s"(m5), [sv] "=&s"(save)
        : [b0] "v"(b0), [b1] "v"(b1), [th] "v"(thr), [c0] "v"(c0), [c1] "v"(c1), [ab] "v"(abase), [one] "v"(one), [off] "n"(OFF)
        : "memory");
  }
}

// The per-tile stream: the reads rb .. rb + n0 of the read arrays, as `total` wave-iterations.
struct Stream { int rb, n0, total; };

// Workgroup shape (developer sweeps: tools/build_variant.sh x -DMIDAS_DIRECT_BLOCK=384).
#ifndef MIDAS_DIRECT_BLOCK
#define MIDAS_DIRECT_BLOCK 256
#endif
constexpr int kDirectBlock = MIDAS_DIRECT_BLOCK;
static_assert(kDirectBlock % 64 == 0 && kDirectBlock >= 128 && kDirectBlock <= 1024, "whole wavefronts");
constexpr int kDirectWavesPerSimd = (kWorkgroupsPerCU * kDirectBlock / 64 + 3) / 4;      // four workgroups per CU


// LPR: the lanes per read where they are a compile-time constant (4: the lane geometry, the phase of four iterations and the DPP
// hand-off are static), 0: whatever DirectParams says, the generic body.
template <int LB, bool BQ0, int OV = kDirectOverhang, int LPR = 0>
__global__ __launch_bounds__(kDirectBlock, kDirectWavesPerSimd) void pileup_direct_kernel(DirectParams p) {
  static_assert(LB == 30 || LB == 32 || LB == 38, "a lane's bases: 8 or 10 words of four base bytes");
  static_assert(LPR == 0 || (LPR == 4 && OV == kDirectOverhang), "static lane geometry: four lanes per read");
  constexpr bool QUAD = LPR == 4;
  constexpr int TILE = kTileSites;
  constexpr int NW = (LB + 3) / 4;          // words of base bytes a lane holds (the last one of LB = 30 / 38: two bytes)
  constexpr int NG = (LB + 7) / 8;          // groups of eight bases (the last one of LB = 30 / 38: six)
  constexpr int KROWS = (LB > 32 ? LB : 32) + 1;      // rows of the byte-mask table: 0 .. LB bases kept
  constexpr int NWAVES = kDirectBlock / 64;
  constexpr int OUT_IT = (TILE + kDirectBlock - 1) / kDirectBlock;
  // OV: sites behind the tile's last that the tallies also hold (see "chunks" below); kDirectOverhangLong for batches of longer reads
  static_assert(OV <= TILE, "the overhang is moved by the write-out's first rounds");
  __shared__ __attribute__((aligned(16))) uint32_t lds[4 * (TILE + OV)];
  __shared__ __attribute__((aligned(16))) uint32_t s_kb[KROWS * NW];    // [h][w]: 0xFF in the bytes of the bases j < h of a lane's NW words
  __shared__ unsigned long long s_stats[MIDAS_STATS];
  __shared__ uint32_t s_next_ticket;
  // [min_match table_len][min_align table_len]; 16-bit entries in the long-overhang instantiation (its reads are <= 288 bases, the
  // thresholds at most that): the kilobyte this saves is what lets FOUR workgroups of it share a CU's 160 KiB
  using table_t = typename std::conditional<(OV > kDirectOverhang), int16_t, int32_t>::type;
  extern __shared__ __attribute__((aligned(16))) uint8_t s_tables_raw[];
  table_t* const s_tables = reinterpret_cast<table_t*>(s_tables_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // Work items.  The tiles [0, n_chunked_tiles) are dealt in CHUNKS of chunk_tiles consecutive tiles, the rest one by one (the
  // chip's last tens of microseconds need the fine grain).  Inside a chunk a read is visited ONCE, by the tile it starts in:
  // what it adds behind that tile's last site lands in the OV sites the tallies hold beyond the tile and moves to the front
  // when the workgroup goes on to the next tile (same contig).  Only a chunk's first tile streams the reads that reach in
  // from the tile before it, as every tile did before (7.5 % of the reads seen twice at 2048 sites and 150 bp; a quarter of
  // that with chunks of four).  The host asks for chunks when the reads are position-sorted; a read that spans more than OV sites
  // (a long deletion, an N skip) makes the chunks it touches fall back to tile-by-tile (chunk_ok), not the batch.
  const int K = p.chunk_tiles > 1 ? p.chunk_tiles : 1;
  const int T4 = K > 1 ? p.n_chunked_tiles : 0;
  const int n4 = T4 / K;
  const int w_end = n4 + (p.n_tiles - T4);              // items
  auto item_first = [&](int i) -> int { return i < n4 ? i * K : T4 + (i - n4); };
  auto item_end = [&](int i) -> int { return i < n4 ? i * K + K : T4 + (i - n4) + 1; };
#ifdef MIDAS_DIRECT_STATIC
  const bool dynamic = false;       // (developer variant: tiles dealt round robin)
#else
  const bool dynamic = (gridDim.x % kSchedGroups) == 0;
#endif
  const int sched_group = (int)(blockIdx.x % kSchedGroups);
  if ((int)blockIdx.x >= w_end) return;
  int c_first = item_first((int)blockIdx.x), c_end = item_end((int)blockIdx.x);      // the chunk in work: tiles [c_first, c_end)
  int i_next = (int)blockIdx.x + (int)gridDim.x;                                      // the item after it (>= w_end: none)
  i_next = i_next < w_end ? i_next : w_end;
#if MIDAS_SNPS_DEBUG_BITS & 256
  unsigned long long pr_cols = 0, pr_bases = 0, pr_work = 0, pr_sync = 0, pr_out = 0, pr_iters = 0;
  const unsigned long long pr_t0 = __builtin_readcyclecounter();
#define PROBE_NOW() __builtin_readcyclecounter()
#else
#define PROBE_NOW() 0ull
#endif

  {
    uint4* z = reinterpret_cast<uint4*>(lds);
    for (int i = tid; i < TILE + OV; i += kDirectBlock) z[i] = make_uint4(0u, 0u, 0u, 0u);
    for (int i = tid; i < p.table_len; i += kDirectBlock) {
      s_tables[i] = (table_t)p.filt->min_match[i];
      s_tables[p.table_len + i] = (table_t)p.filt->min_align[i];
    }
    for (int i = tid; i < KROWS * NW; i += kDirectBlock) {
      const int h = i / NW, wd = i - h * NW;
      uint32_t kb = 0;
      for (int k = 0; k < 4; ++k)
        if (4 * wd + k < h) kb |= 0xFFu << (8 * k);
      s_kb[i] = kb;
    }
    if (tid < MIDAS_STATS) s_stats[tid] = 0ull;
  }

  const int lpr = QUAD ? 4 : p.lanes_per_read;
  const int rpw = QUAD ? 16 : p.reads_per_wave;
  const int g = lane / lpr;
  const int c = lane - g * lpr;
  const int q0 = c * LB;                           // first base of the lane in the read's stored query
  const uint32_t lds_base = (uint32_t)(size_t)(__attribute__((address_space(3))) void*)lds;
  // a base counts iff its byte >= thr (layout.h dense_threshold: 52 for every baseq <= 0 -- every A/C/G/T base, no N, no masked slot)
  const uint32_t thr = BQ0 ? dense_threshold(0) : dense_threshold(p.baseq);
  const int rq = p.readq < 0 ? 0 : (p.readq > 256 ? 256 : p.readq);   // sum(q) < rq * l  <=>  np.mean(q) < readq (q <= 255)
  const uint32_t one = 1u;
  const int table_len = own_scalar(p.table_len), mapq_min = own_scalar(p.mapq_min);

  // (cin: the tile continues a chunk in its contig -- the reads that reach in from the tile before were tallied by that tile)
  auto load_stream = [&](ParamsAgain q, int tt, bool cin) -> Stream {
    const ConstWords c_tb = (ConstWords)(size_t)q->tbegin;
    const ConstWords c_te = (ConstWords)(size_t)q->tend;
    Stream s;
    const uint32_t b = cin ? c_te[tt - 1] : c_tb[tt], e = c_te[tt];
    s.rb = e > b ? (int)b : 0;
    s.n0 = e > b ? (int)(e - b) : 0;
    s.total = (s.n0 + rpw - 1) / rpw;
    return s;
  };
  // reads of a stream's wave-iteration `it` (wave-uniform): the lanes with g below it hold one
  auto reads_in = [&](const Stream& st, int it) -> int {
    const long long left = (long long)st.n0 - (long long)it * rpw;
    return left <= 0 ? 0 : (left < rpw ? (int)left : rpw);
  };

  // The lanes `go` tally bases [lo, hi) of their LB, the first of the lane at tile-relative site loc0, group by group of
  // eight.  Partial lanes zero the bytes outside [lo, hi) (a zero byte never counts): two rows of the byte-mask table (LDS).
  // (sparse: a pass with few lanes, e.g. the one lane of a read that holds its indel -- a group of eight bases none of the
  // wave's lanes has a base in is skipped)
  auto tally_range = [&](bool go, int lo, int hi, int loc0, const uint32_t (&bv)[NW], auto sparse_tag) {
    constexpr bool SPARSE = decltype(sparse_tag)::value;
    const uint32_t abase = ((uint32_t)loc0 << 4) + lds_base;
    const bool masked = !(kDebug & 32) && __ballot(go && (lo > 0 || hi < LB)) != 0ull;   // partial lanes: the bytes outside become 0
    unsigned long long gmask[NG];
    if (SPARSE) {
#pragma unroll
      for (int S = 0; S < NG; ++S) gmask[S] = __ballot(go && lo < 8 * S + 8 && hi > 8 * S);
    }
    if (!go) return;
    const uint32_t* const row_hi = s_kb + NW * (hi > KROWS - 1 ? KROWS - 1 : hi);      // bytes [lo, hi): row hi less row lo
    const uint32_t* const row_lo = s_kb + NW * (lo < 0 ? 0 : lo);
    auto group = [&](auto sidx, auto nbases) {
      constexpr int S = decltype(sidx)::value;
      if (SPARSE && gmask[S] == 0ull) return;
      uint32_t x0 = bv[2 * S], x1 = bv[2 * S + 1];
      if (masked) {
        const uint2 kh = *reinterpret_cast<const uint2*>(row_hi + 2 * S);
        const uint2 kl = *reinterpret_cast<const uint2*>(row_lo + 2 * S);
        x0 &= kh.x & ~kl.x;
        x1 &= kh.y & ~kl.y;
      }
      tally_group<128 * S, decltype(nbases)::value>(x0, x1, thr, abase, one);
    };
    using std::integral_constant;
    group(integral_constant<int, 0>{}, integral_constant<int, 8>{});
    group(integral_constant<int, 1>{}, integral_constant<int, 8>{});
    group(integral_constant<int, 2>{}, integral_constant<int, 8>{});
    group(integral_constant<int, 3>{}, integral_constant<int, (NG > 4 ? 8 : LB - 24)>{});
    if constexpr (NG > 4) group(integral_constant<int, 4>{}, integral_constant<int, LB - 32>{});
  };

  // ---- phases.  What a read needs done ONCE -- its CIGAR's shape, the two filter tables, keep_read, its count in the species'
  // counters, its error -- is done by ONE lane for it, for a PHASE of up to PH of the wave's iterations at a time (PH * rpw <= 64
  // reads: four iterations of 16 reads of four lanes), and not by each of its lanes in each iteration: a wave instruction costs
  // the same for 16 useful lanes as for 64.  The lane that owns read `og` of the phase's iteration `oj` loads the read's record,
  // its first four CIGAR ops and its quality sum, and packs what the lanes with the read's bases need into four words (Desc);
  // they fetch them in their iteration -- with four lanes per read the owner of read g of iteration j is lane 4 g + j, and the
  // fetch is a DPP quad_perm:[j,j,j,j] move (j static in the unrolled body: nothing goes through the LDS pipeline); any other
  // lane count: lane j * rpw + g and ds_bpermute_b32.  A phase never straddles a tile.  PH is even where two iterations fit
  // (the two sets of base registers keep their roles inside a tile); with one lane per read a phase is one iteration.
  const int ph_fit = 64 / rpw;
  const int PH = QUAD ? 4 : (ph_fit >= 4 ? 4 : (ph_fit >= 2 ? 2 : 1));
  const bool quad = QUAD || lpr == 4;
  // (one register: the iteration oj of its phase and the read og of that iteration this lane owns, as the read's place among the
  // wave's reads of the phase's tile, oj * NWAVES * rpw + og, with oj in the top byte)
  const uint32_t own_slot = quad ? (uint32_t)((lane & 3) * NWAVES * rpw + (lane >> 2)) | ((uint32_t)(lane & 3) << 24)
                                 : (uint32_t)((lane / rpw) * NWAVES * rpw + lane % rpw) | ((uint32_t)(lane / rpw) << 24);
  const bool lane_on = QUAD || g < rpw;                                  // (64 % lpr lanes at the wave's end never hold a read)
  // iterations of the phase that opens with `rem` of the wave's iterations of a tile left: PH, but 2 + 3 for the last five of PH =
  // 4 (not 4 + 1: a phase of at least two iterations requests the next phase's CIGARs a whole iteration ahead of their use)
  auto phase_len = [&](int rem) -> int { return (PH == 4 && rem == 5) ? 2 : (rem < PH ? rem : PH); };
  auto wave_its = [&](const Stream& s) -> int { return s.total > wave ? (s.total - wave + NWAVES - 1) / NWAVES : 0; };

  // ---- loads.  NO load sits in a branch of the iteration's body -- a lane without a read fetches read 0's record, a lane without
  // bases the first bytes of the iteration's payload -- so that the compiler can count the loads in flight (a load in a branch
  // makes it wait for every outstanding load, vmcnt(0), before the first use of any of them: the prefetch of the next
  // iteration's bases would be waited for at once).
  //   nmq: NM (16 bits, 0xFFFF = no NM tag) | mapq << 16      l_nc: l_seq | n_cigar << 16
  struct Raw { uint32_t pos, l_nc, nmq, off; };
  const uint4* const recs = reinterpret_cast<const uint4*>(p.rec);
  // the record of this lane's read in wave-iteration `it` of a tile's stream: ONE dwordx4, of which the base loads of the iteration
  // take the payload offset and the lengths (two iterations ahead of the iteration, as the phases' own loads are not)
  auto fetch = [&](const Stream& st, int it) -> Raw {
    const uint32_t v = (uint32_t)(it * rpw) + (uint32_t)g;       // (a stream holds fewer than 2^31 reads, it * rpw <= n0 + 63)
    const uint32_t r = v < (uint32_t)st.n0 ? (uint32_t)st.rb + v : 0u;
    const uint4 x = recs[r];
    Raw f;
    f.pos = x.x; f.l_nc = x.y; f.nmq = x.z; f.off = x.w;
    return f;
  };
  // the lane's bases (two 16-byte loads of base bytes, and an 8-byte one behind them for 38 bases: the payload's slack covers
  // what the read's last lane fetches behind it), off ONE scalar base -- the payload of the iteration's first read (lane 0's) --
  // plus a 32-bit lane offset: the reads of an iteration are neighbours in the payload.
  auto settle = [&](const Raw& f, int n_reads_it, uint32_t (&b)[NW]) {
    const bool act = g < n_reads_it;
    const uint32_t l_nc = act ? f.l_nc : 0u;
    const uint32_t off0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)f.off);        // (lane 0: the iteration's first read, or read 0)
    const uint8_t* const base = p.payload + ((unsigned long long)off0 << 3);
    const uint32_t l = l_nc & 0xFFFFu, nc4 = (l_nc >> 16) << 2;
    const uint32_t rel = (f.off - off0) << 3;                          // (an iteration's reads lie within a few hundred KB)
    const bool has = (uint32_t)q0 < l && !(kDebug & 128);
    const uint32_t vb = has ? rel + nc4 + 4u + (uint32_t)q0 : 0u;
    const u32x4_a1 ba = *reinterpret_cast<const u32x4_a1*>(base + (size_t)vb);
    const u32x4_a1 bb = *reinterpret_cast<const u32x4_a1*>(base + (size_t)vb + 16);
    b[0] = ba.x; b[1] = ba.y; b[2] = ba.z; b[3] = ba.w;
    b[4] = bb.x; b[5] = bb.y; b[6] = bb.z; b[7] = bb.w;
    if constexpr (NW > 8) {
      const u32x2_a1 bc = *reinterpret_cast<const u32x2_a1*>(base + (size_t)vb + 32);
      b[8] = bc.x; b[9] = bc.y;
    }
  };
  // the record of the read this lane OWNS in the phase of `n` iterations that opens with the wave's k0-th of a stream ...
  auto owned = [&](const Stream& s, int k0, int n, uint32_t* idx) -> bool {
    const uint32_t v = (uint32_t)((wave + k0 * NWAVES) * rpw) + (own_slot & 0xFFFFFFu);
    *idx = (uint32_t)s.rb + v;
    return (int)(own_slot >> 24) < n && v < (uint32_t)s.n0;
  };
  auto fetch_phase = [&](const Stream& s, int k0, int n) -> Raw {
    uint32_t idx;
    const bool on = owned(s, k0, n, &idx);
    const uint4 x = recs[on ? idx : 0u];
    Raw f;
    f.pos = x.x; f.l_nc = x.y; f.nmq = x.z; f.off = x.w;
    return f;
  };
  // ... and, addressed from it, the read's first four CIGAR ops (one 16-byte load; the payload has slack behind its last read) and
  // its quality sum (one dword)
  struct Own { uint32_t cg[4]; uint32_t qs; };
  auto gather = [&](const Raw& f, Own& o) {
    const uint8_t* const rp = p.payload + ((unsigned long long)f.off << 3);
    const u32x4_a4 cv = *reinterpret_cast<const u32x4_a4*>(rp);
    const uint32_t qs = *reinterpret_cast<const uint32_t*>(rp + (size_t)((f.l_nc >> 16) << 2));
    o.cg[0] = cv.x; o.cg[1] = cv.y; o.cg[2] = cv.z; o.cg[3] = cv.w;
    o.qs = qs;
  };
  // What the owner hands to the lanes of a read it keeps (all zero for any other):
  //   d0 pos    d1 l_seq | lead << 11 | kept << 22    d2 m1 | alen << 16    d3 gap | (the gap is an insertion) << 16
  // (l_seq and the clip are at most kMaxLSeq = 1024, a deletion or skip at most kMaxFastGap: direct_common.h ReadShape)
  struct Desc { uint32_t d0, d1, d2, d3; };

  Tile tile = load_tile((ConstWords)(size_t)p.tiles, c_first);
  Stream st = load_stream(params_again(), c_first, false);
  // The pipeline of a wave.  Bases: two register sets that swap roles every iteration (the phase's body is unrolled: a copy at a
  // back edge would have to WAIT for the loads it copies -- the next iteration's bases, requested a moment ago):
  //   set A / B   one holds the iteration being tallied, the other the next one's bases (in flight)
  //   raw X       the record of the iteration after that (in flight); its bases are requested at the top of the next body
  // Between tiles, and at the start of every phase, the current iteration sits in set A.  Per-read work:
  //   desc        the descriptors of the phase in work, one read per lane
  //   raw N, own N   the records (requested at the start of the phase in work) and CIGARs / quality sums (requested at the top
  //               of its second iteration) of the NEXT phase's reads
  Raw rawX, rawN;
  Own ownN;
  Desc desc;
  int nrX = 0;                                  // reads of the iteration the record X belongs to (wave-uniform)
  uint32_t bA[NW], bB[NW];
  {
    const Raw r0 = fetch(st, wave);
    rawX = fetch(st, wave + NWAVES);
    nrX = reads_in(st, wave + NWAVES);
    rawN = fetch_phase(st, 0, phase_len(wave_its(st)));
    settle(r0, reads_in(st, wave), bA);
    gather(rawN, ownN);
  }
  __syncthreads();   // LDS zeroed, tables in place

  uint32_t acc_cov = 0u;                 // (a thread's sites between two flushes: far below 2^32)
  unsigned long long acc_depth = 0ull;
  int t = c_first;
  for (;;) {
    // (what the stream loop uses of the tile: scalars of their own, not parts of the eight words the tile was loaded in)
    const int tile_len = own_scalar(tile.len), tile_start = own_scalar(tile.start), contig_len = own_scalar(tile.contig_len);
    // the tile after this one: the chunk's next, or the next item's first
    const bool in_chunk = t + 1 < c_end;
    const bool more = in_chunk || i_next < w_end;
    const int wn = in_chunk ? t + 1 : (more ? item_first(i_next) : t);
    // (a chunk that holds -- or is reached by -- a read spanning more than the overhang is piled up tile by tile: chunk_ok)
    const ParamsAgain pt = params_again();
    const ConstWords c_tiles = (ConstWords)(size_t)pt->tiles;
    const uint8_t* const chunk_ok = pt->chunk_ok;
    const bool carry = in_chunk && (!chunk_ok || chunk_ok[c_first / K] != 0);
    const bool cout = carry && (int32_t)c_tiles[8 * (size_t)wn] == tile.contig;      // its first OV sites are tallied here
    // (the contig's last tile may be shorter than the overhang: nothing is tallied behind the contig's end)
    const int next_len = (int32_t)c_tiles[8 * (size_t)wn + 2];
    const int ext_len = tile_len + (cout ? (next_len < OV ? next_len : OV) : 0);
    const int it_hi = st.total;
    uint32_t w_aligned = 0, w_mapped = 0;
    constexpr int REF_IT = (TILE + 4 * kDirectBlock - 1) / (4 * kDirectBlock);

    // the column / base prefetch runs across the tile boundary (as in pileup_tiles.hip): a wave's last two iterations fetch
    // the columns of its first two iterations of the NEXT tile
    const int n_w = it_hi > wave ? (it_hi - wave + NWAVES - 1) / NWAVES : 0;
    const bool xt = more && n_w >= 2;
    Stream xs = st;
    if (xt) xs = load_stream(pt, wn, cout);
    // The stream the iterations' records are being fetched from: this tile's, and from where the prefetch crosses into the next
    // tile the next tile's -- switched ONCE there (cross_if_due, between two iterations), not selected in every iteration.
    //   f_left  fetches until the prefetch crosses
    //   f, f_i  the stream and its wave-iteration to fetch next -- or, with the static lane geometry (a vector register for a scalar one):
    //   f_rec   per lane: the index of the record it fetches next, rb + it * rpw + g (one add an iteration)
    //   f_end   the stream's end, rb + n0: a lane at or behind it has no read (it fetches record 0)
    //   f_rem   reads of the stream from the iteration to fetch onwards, n0 - it * rpw (may be <= 0)
    // (the wave's iterations 0 and 1 of this tile are in the pipeline: n_w - 2 more of this tile, if the prefetch crosses at all;
    // a stream holds fewer than 2^31 reads and it * rpw <= n0 + 63 + 2 * kDirectBlock)
    constexpr int f_step = NWAVES * 16;
    Stream f = st;
    int f_i = 0;
    uint32_t f_rec = 0u;
    int f_end = 0, f_rem = 0;
    auto fetch_from = [&](const Stream& s, int it) {
      if constexpr (QUAD) {
        f_rec = (uint32_t)s.rb + (uint32_t)(it * 16) + (uint32_t)g;
        f_end = s.rb + s.n0;
        f_rem = s.n0 - it * 16;
      } else {
        f.rb = s.rb; f.n0 = s.n0;
        f_i = it;
      }
    };
    fetch_from(st, wave + 2 * NWAVES);
    int f_left = xt ? n_w - 2 : 0x7FFFFFFF;
    auto cross_if_due = [&]() {
      if (f_left == 0) {
        fetch_from(xs, wave);
        f_left = -1;
        asm volatile("");      // (a branch, not selects: the next stream's scalars are read here only)
      }
    };
    cross_if_due();
    // ---- a read walked op by op (the slow path), by the lanes that would hold its bases.  Rare: what the lanes need -- record,
    // CIGAR, quality sum, bases -- they fetch here, by the read's index; keep_read with every test evaluated and the reference's
    // order of outcomes, counters and error of its own.
    // (bw: a set of base registers that is free -- at the start of a phase set B holds nothing yet)
    auto walk = [&](bool slow, uint32_t idx, uint32_t (&bw)[NW]) {
      const DirectRec rc = p.rec[slow ? idx : 0u];
      const int pos = rc.pos;
      const int l = slow ? (int)(rc.l_nc & 0xFFFFu) : 0;
      const uint32_t nc = slow ? rc.l_nc >> 16 : 0u;
      const uint8_t* const rp = p.payload + ((unsigned long long)rc.off8 << 3);
      CigarView cg;
      cg.load(reinterpret_cast<const uint32_t*>(rp));
      uint32_t qsum = *reinterpret_cast<const uint32_t*>(rp + (size_t)(nc << 2));
      const int nb = l - q0 < LB ? (l - q0 < 0 ? 0 : l - q0) : LB;     // bases of the read in this lane
      const bool has = nb > 0;
      const uint8_t* const bp = has ? rp + (size_t)(nc << 2) + 4u + (size_t)q0 : rp;
      {
        const u32x4_a1 ba = *reinterpret_cast<const u32x4_a1*>(bp);
        const u32x4_a1 bb = *reinterpret_cast<const u32x4_a1*>(bp + 16);
        bw[0] = ba.x; bw[1] = ba.y; bw[2] = ba.z; bw[3] = ba.w;
        bw[4] = bb.x; bw[5] = bb.y; bw[6] = bb.z; bw[7] = bb.w;
        if constexpr (NW > 8) {
          const u32x2_a1 bc = *reinterpret_cast<const u32x2_a1*>(bp + 32);
          bw[8] = bc.x; bw[9] = bc.y;
        }
      }
      if (kDebug & 64) qsum = 0x00FFFFFFu;
      const bool t_noqual = (qsum & kDenseQualAbsent) != 0u;
      qsum &= ~kDenseQualAbsent;
      const uint32_t nm16 = rc.nmq & 0xFFFFu;
      const int nm = (int)nm16, mapq = (int)((rc.nmq >> 16) & 0xFFu);
      const uint32_t ncs = nc;
      // [EXT] pysam query_alignment_start / _end -> len(aln.query_alignment_sequence) (midas/run/snps.py:145)
      long long qs = 0, qe = 0;
      query_bounds(cg, ncs, l, &qs, &qe);
      long long al = qe - qs;
      al = al < 0 ? 0 : (al > 2047 ? 2047 : al);      // (l_seq <= 1024)
      const int align_g = (int)al;
      // the one case in which count_coverage raises IndexError for a kept read: a match op maps a query position >= l_seq
      // onto a site inside the contig
      bool t_over = false;
      {
        long long qpos = 0, rpos = pos;
        const long long clen = tile.contig_len;
        for_each_op(cg, ncs, [&](uint32_t, uint32_t v) {
          const uint32_t op = v & 15u;
          const long long len = (long long)(v >> 4);
          if (op_is_match(op)) {
            if (qpos + len > (long long)l) {
              const long long qs2 = qpos > (long long)l ? qpos : (long long)l;
              const long long rs = rpos + (qs2 - qpos), re = rpos + len;
              if (rs < clen && re > 0) t_over = true;
            }
            qpos += len;
            rpos += len;
          } else if (op == OP_I || op == OP_S || (op == OP_P && p.pad_advances)) {
            qpos += len;
          } else if (op == OP_D || op == OP_N) {
            rpos += len;
          }
          return true;
        });
      }
      // ---- keep_read, every test evaluated, the reference's order decides which outcome wins ---------------------------
      const int min_match = s_tables[align_g < table_len ? align_g : 0];
      const int min_align = s_tables[table_len + (l < table_len ? l : 0)];
      const bool t_noseq = l == 0;
      const bool t_nonm = nm16 == 0xFFFFu;
      const bool t_zero = align_g == 0;
      const bool t_pid = align_g - nm < min_match;
      const bool t_drop = ((int)qsum < rq * l) | (mapq < mapq_min) | (align_g < min_align);
      uint32_t e = t_over ? (uint32_t)E_CIGAR_OVERRUN : 0u;
      e = t_drop ? 0u : e;
      e = t_noqual ? (uint32_t)E_NO_QUAL : e;
      e = t_pid ? 0u : e;
      e = t_zero ? (uint32_t)E_ZERO_ALIGN : e;
      e = t_nonm ? (uint32_t)E_NO_NM : e;
      e = t_noseq ? (uint32_t)E_NO_SEQ : e;
      const bool keep_s = slow && !(t_noseq | t_nonm | t_zero | t_pid | t_noqual | t_drop | t_over);
      // owner tile of a read = the tile holding its (clamped) start: it alone counts the read in the stats
      int cpos = pos < 0 ? 0 : pos;
      cpos = cpos > tile.contig_len - 1 ? tile.contig_len - 1 : cpos;
      const bool owner_s = slow && cpos >= tile_start && cpos < tile_start + tile_len && !(tile.halo && pos < 0);
      const int rel = pos - tile_start;                                     // may wrap for absurd positions:
      int rrel = (rel > (1 << 25) || rel < -(1 << 30)) ? (1 << 25) : rel;   // those are parked far right
      // ---- CIGAR walk ([EXT] get_aligned_pairs(matches_only=True)): one match segment at a time ------------------------
      // 32-bit saturating positions: a query position only matters below q1 <= 1024 and a tile-relative reference
      // position only below 4096, and both only ever grow.
      uint32_t k = 0;
      int qpos = 0, jlo = 0, jhi = 0, loc0 = 0;
      const int q1 = q0 + nb;
      auto next_segment = [&]() -> bool {
        while (k < nc) {
          const uint32_t v = cg[k];
          ++k;
          const uint32_t op = v & 15u;
          const int len = (int)(v >> 4);
          const bool m = consumes_both(op);
          bool found = false;
          if (m) {
            const int lo = qpos > q0 ? qpos : q0;
            const int hi = (qpos + len) < q1 ? (qpos + len) : q1;
            found = lo < hi;
            if (found) { jlo = lo - q0; jhi = hi - q0; loc0 = rrel + (q0 - qpos); }
          }
          if (m || op == OP_I || op == OP_S || (op == OP_P && p.pad_advances)) { qpos += len; qpos = qpos > (1 << 29) ? (1 << 29) : qpos; }
          if (m || op == OP_D || op == OP_N) { rrel += len; rrel = rrel > (1 << 29) ? (1 << 29) : rrel; }
          if (found) return true;   // H, P and anything else: no effect
        }
        return false;
      };
      bool walking = keep_s && has;
      if (walking) walking = next_segment();
      while (__ballot(walking) != 0ull) {
        const int lo = jlo > -loc0 ? jlo : -loc0;
        const int hi = jhi < ext_len - loc0 ? jhi : ext_len - loc0;
        if (!(kDebug & 1)) tally_range(walking && lo < hi, lo, hi, loc0, bw, std::true_type{});
        walking = (walking && k < nc) ? next_segment() : false;
      }
      const bool head = owner_s && c == 0;
      w_aligned += (uint32_t)__popcll(__ballot(head));
      w_mapped += (uint32_t)__popcll(__ballot(head && keep_s));
      // (a read of the piece in front, midas_snps_contigs.origin: its own piece reports what keep_read raises, this one the
      // overrun its walk runs into here)
      const bool walk_err = slow && tile.halo && pos < 0 && c == 0 && e == (uint32_t)E_CIGAR_OVERRUN;
      if ((head && e) || walk_err) atomicMin(p.err, ((unsigned long long)idx << 8) | e);
    };

    // ---- the start of a phase of n_ph iterations, the wave's k0-th onwards: every owner its read, from raw N / own N (requested
    // in the phase before, or in front of the tile).  Then the records of the phase after it are requested: the next of this
    // tile, or the first of the next tile's stream (`xs`, as the bases' look-ahead).
    auto open_phase = [&](int k0, int n_ph, const Stream& nf, int nf_k, int nf_len) {
      MIDAS_MARK("phase");
      uint32_t idx;
      const bool act = owned(st, k0, n_ph, &idx);
      const int pos = (int)rawN.pos;
      const int l = act ? (int)(rawN.l_nc & 0xFFFFu) : 0;
      const uint32_t nc = act ? rawN.l_nc >> 16 : 0u;
      // (developer timing variant, bit 512: ALL per-read work off -- no quality sum, no CIGAR shape, no filter tables: every read is
      // one match run of its length and kept; the tallies and the stream stay)
      // The read's quality sum travels with it (layout.h: bit 31 QUAL absent); sum(q) < readq * l_seq is np.mean(q) < readq exactly.
      uint32_t qsum = (kDebug & (64 | 512)) ? 0x00FFFFFFu : ownN.qs;
      const bool t_noqual = (qsum & kDenseQualAbsent) != 0u;
      qsum &= ~kDenseQualAbsent;
      const uint32_t nm16 = rawN.nmq & 0xFFFFu;
      const int nm = (int)nm16, mapq = (int)((rawN.nmq >> 16) & 0xFFu);
      // ---- the read's shape: one match op of the read's length settles most reads; anything else takes the four-op grammar
      // (wave-uniform branch) -----------------------------------------------------------------------------------------------
      MIDAS_MARK("shape");
      ReadShape sh;
      sh.lead = 0u; sh.m1 = (uint32_t)l; sh.ins = 0u; sh.del = 0u; sh.alen = (uint32_t)l;
      bool shaped = nc == 1u && op_is_match(ownN.cg[0] & 15u) && (ownN.cg[0] >> 4) == (uint32_t)l && l >= 1;
      if (kDebug & 512) shaped = true;
      if (__ballot(act && !shaped) != 0ull) {
        ReadShape s2;
        const bool ok = decode_shape(ownN.cg[0], ownN.cg[1], ownN.cg[2], ownN.cg[3], nc, (uint32_t)l, &s2);
        if (!shaped) { sh = s2; shaped = ok; }
      }
      // one or two match runs, NM present, the start inside the contig: the fast path.  Everything else is walked.
      const bool fast = act && shaped && nm16 != 0xFFFFu && pos >= 0 && pos < contig_len;
      const bool slow = act && !fast;
      // ---- keep_read (midas/run/snps.py:141-162): a fast read has SEQ, NM and a non-empty aligned part -------------------------
      MIDAS_MARK("filter");
      const int align_len = (int)sh.alen;
      const int min_match = (kDebug & 512) ? 0 : s_tables[align_len < table_len ? align_len : 0];
      const int min_align = (kDebug & 512) ? 0 : s_tables[table_len + (l < table_len ? l : 0)];
      const bool t_pid = align_len - nm < min_match;                                                       // pid < mapid
      const bool t_drop = ((int)qsum < rq * l) | (mapq < mapq_min) | (align_len < min_align);             // readq, mapq, aln_cov
      const uint32_t err = (fast && !t_pid && t_noqual) ? (uint32_t)E_NO_QUAL : 0u;
      const bool keep = fast && !(t_pid | t_noqual | t_drop);
      const int rel = pos - tile_start;            // 0 <= pos < contig length: no wrap
      const bool owner = fast && rel >= 0 && rel < tile_len;
      const uint32_t gap = sh.ins ? sh.ins : sh.del;
      desc.d0 = (uint32_t)pos;
      desc.d1 = keep ? ((uint32_t)l | (sh.lead << 11) | (1u << 22)) : 0u;
      desc.d2 = sh.m1 | (sh.alen << 16);
      desc.d3 = gap | (sh.ins ? 1u << 16 : 0u);
      // ---- per-species read counters: one ballot pair per phase ------------------------------------------------------------
      MIDAS_MARK("counters");
      w_aligned += (uint32_t)__popcll(__ballot(owner));
      w_mapped += (uint32_t)__popcll(__ballot(owner && keep));
      rawN = fetch_phase(nf, nf_k, nf_len);    // the records of the phase after this one (nf: the stream they are in)
      MIDAS_MARK("slowgate");
      if (owner && err) atomicMin(params_again()->err, ((unsigned long long)idx << 8) | err);      // (rare: a kept read without qualities)
      const unsigned long long slow_mask = __ballot(slow);
      if (slow_mask != 0ull) {
        for (int j = 0; j < n_ph; ++j) {
          const int ol = quad ? 4 * g + j : j * rpw + g;
          const bool mine = lane_on && ((slow_mask >> (ol & 63)) & 1ull) != 0ull;
          if (__ballot(mine) != 0ull) walk(mine, (uint32_t)(st.rb + (wave + (k0 + j) * NWAVES) * rpw + g), bB);
        }
      }
      MIDAS_MARK("phaseend");
    };

    // one wave-iteration, the J-th of its phase and the wave's k_it-th of the tile: tallies the bases b_cur, requests the bases
    // of the next iteration into b_n from the record rawX and then the record of the one after it into rawX
    auto iteration = [&](auto jtag, int k_it, uint32_t (&b_cur)[NW], uint32_t (&b_n)[NW]) {
      constexpr int J = decltype(jtag)::value;
      const unsigned long long pt0 = PROBE_NOW();
      (void)pt0;
      MIDAS_MARK("settle");
      settle(rawX, nrX, b_n);                  // (the record of the next iteration has arrived: its bases are requested ...)
      // ... then the record of the one after it (the wave's k_it + 2 nd of this tile, or counted on into the next tile's stream)
      if constexpr (QUAD) {
        const uint4 x = recs[f_rec < (uint32_t)f_end ? f_rec : 0u];
        rawX.pos = x.x; rawX.l_nc = x.y; rawX.nmq = x.z; rawX.off = x.w;
        nrX = f_rem <= 0 ? 0 : (f_rem < 16 ? f_rem : 16);
        f_rec += (uint32_t)f_step;
        f_rem -= f_step;
      } else {
        rawX = fetch(f, f_i);
        nrX = reads_in(f, f_i);
        f_i += NWAVES;
      }
      f_left -= 1;
      if constexpr (J == 1) gather(rawN, ownN);      // (the next phase's records, requested an iteration ago, have arrived)
#if MIDAS_SNPS_DEBUG_BITS & 256
      const unsigned long long pt1 = PROBE_NOW();
      asm volatile("" :: "v"(b_cur[0]), "v"(b_cur[NW - 1]));
      const unsigned long long pt2 = PROBE_NOW();
      pr_cols += pt1 - pt0; pr_bases += pt2 - pt1; pr_iters += 1;
#endif

      if (kDebug & 4) {          // (developer timing variant: the stream of loads only)
        asm volatile("" :: "v"(b_cur[0]), "v"(b_cur[NW - 1]), "v"(desc.d0));
        cross_if_due();
        return;
      }
      // ---- the read's descriptor, from its owner -----------------------------------------------------------------------------
      MIDAS_MARK("handoff");
      uint32_t d0, d1, d2, d3;
      if (quad) {
        d0 = quad_take<J>(desc.d0); d1 = quad_take<J>(desc.d1); d2 = quad_take<J>(desc.d2); d3 = quad_take<J>(desc.d3);
      } else {
        const int src = (J * rpw + g) << 2;
        d0 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)desc.d0);
        d1 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)desc.d1);
        d2 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)desc.d2);
        d3 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)desc.d3);
      }
      // ======================= one or two gap-free match runs ==================================================================
      MIDAS_MARK("clip");
      const bool keep = lane_on && ((d1 >> 22) & 1u) != 0u;
      const int pos = (int)d0;
      const int l = (int)(d1 & 0x7FFu), lead = (int)((d1 >> 11) & 0x7FFu);
      const int m1 = (int)(d2 & 0xFFFFu), align_len = (int)(d2 >> 16);
      const int gapl = (int)(d3 & 0xFFFFu);
      const int ins = (d3 >> 16) ? gapl : 0, del = (d3 >> 16) ? 0 : gapl;
      const int nb = l - q0 < LB ? (l - q0 < 0 ? 0 : l - q0) : LB;     // bases of the read in this lane
      {
        const int rel = pos - tile_start;            // 0 <= pos < contig length: no wrap
        // run A: query [lead, lead + m1) at sites pos ...; run B: query [lead + m1 + ins, lead + alen) at pos + m1 + del ...
        // -- this lane's part of each, clipped to the tile
        const int qa1 = lead + m1, qb0 = qa1 + ins, qb1 = lead + align_len;
        const int loc_a = rel + (q0 - lead);
        const int loc_b = loc_a + del - ins;
        int lo_a = lead - q0, hi_a = qa1 - q0, lo_b = qb0 - q0, hi_b = qb1 - q0;
        lo_a = lo_a > -loc_a ? lo_a : -loc_a;
        lo_a = lo_a > 0 ? lo_a : 0;
        hi_a = hi_a < ext_len - loc_a ? hi_a : ext_len - loc_a;
        hi_a = hi_a < nb ? hi_a : nb;
        lo_b = lo_b > -loc_b ? lo_b : -loc_b;
        lo_b = lo_b > 0 ? lo_b : 0;
        hi_b = hi_b < ext_len - loc_b ? hi_b : ext_len - loc_b;
        hi_b = hi_b < nb ? hi_b : nb;
        const bool go_a = keep && lo_a < hi_a, go_b = keep && lo_b < hi_b;
        // first pass: every lane its run (the lane that holds the indel: the part in front of it); second pass, only when a
        // lane of the wave has bases on both sides of an indel: the part behind it
        const bool go1 = go_a | go_b;
        MIDAS_MARK("pass1");
        if (!(kDebug & 1) && __ballot(go1) != 0ull)
          tally_range(go1, go_a ? lo_a : lo_b, go_a ? hi_a : hi_b, go_a ? loc_a : loc_b, b_cur, std::false_type{});
        const bool go2 = go_a & go_b;
        MIDAS_MARK("pass2");
        if (!(kDebug & (1 | 16)) && __ballot(go2) != 0ull) tally_range(go2, lo_b, hi_b, loc_b, b_cur, std::true_type{});
      }
      MIDAS_MARK("iterend");
#if MIDAS_SNPS_DEBUG_BITS & 256
      pr_work += PROBE_NOW() - pt2;
#endif
      cross_if_due();
    };
    {
      using std::integral_constant;
      int k0 = 0;
      while (k0 < n_w) {
        const int n_ph = phase_len(n_w - k0);
        // the phase after this one: the next of this tile, or -- behind the tile's last -- the first of the next tile's stream
        Stream nf = st;
        int nf_k = k0 + n_ph, nf_len = phase_len(n_w - nf_k);
        if (xt && nf_k >= n_w) {
          nf.rb = xs.rb; nf.n0 = xs.n0;
          nf_k = 0;
          nf_len = phase_len(wave_its(xs));
          asm volatile("");
        }
        open_phase(k0, n_ph, nf, nf_k, nf_len);
        iteration(integral_constant<int, 0>{}, k0, bA, bB);
        if (n_ph > 1) {
          iteration(integral_constant<int, 1>{}, k0 + 1, bB, bA);
          if (n_ph > 2) {
            iteration(integral_constant<int, 2>{}, k0 + 2, bA, bB);
            if (n_ph > 3) iteration(integral_constant<int, 3>{}, k0 + 3, bB, bA);
          }
        } else {
          gather(rawN, ownN);      // (a phase of one iteration: a tile that gives the wave one, or an odd tail of phases of two)
          // one lane per read: a phase IS an iteration, and every one of them tallies set A (the copy waits for bases that the
          // next phase's wait for its CIGARs, requested behind them, covers anyway)
          if (PH == 1) {
#pragma unroll
            for (int w = 0; w < NW; ++w) bA[w] = bB[w];
          }
        }
        k0 += n_ph;
      }
      if ((n_w & 1) && PH != 1) {  // (once per tile, not per iteration)
#pragma unroll
        for (int w = 0; w < NW; ++w) bA[w] = bB[w];
      }
    }

    // the tile's reference letters: requested here, behind the stream loop (two registers less in it), they arrive while
    // the workgroup waits for its last wave and writes the counts out
    MIDAS_MARK("refletters");
    const ParamsAgain pe = params_again();
    uint8_t* const out_allele = pe->out_allele;
    uint32_t refw[REF_IT];
    if (out_allele) {
      const uint8_t* ref = pe->ref + tile.site_base;
#pragma unroll
      for (int it = 0; it < REF_IT; ++it) {
        const int i = 4 * (tid + it * kDirectBlock);
        if (i + 4 <= tile_len) refw[it] = *reinterpret_cast<const u32_a1*>(ref + i);
      }
    }
    if (lane == 0) {
      if (w_aligned) atomicAdd(&s_stats[MIDAS_STAT_ALIGNED], (unsigned long long)w_aligned);
      if (w_mapped) atomicAdd(&s_stats[MIDAS_STAT_MAPPED], (unsigned long long)w_mapped);
    }
    // ---- next tile ---------------------------------------------------------------------------------------------------------
    MIDAS_MARK("nexttile");
    const int tn = wn;
    const Tile ntile = load_tile((ConstWords)(size_t)pe->tiles, tn);
    const Stream nst = load_stream(pe, tn, cout);
    const bool take = more && !in_chunk;          // the next tile opens the next item: draw the one after it
    const unsigned long long ps0 = PROBE_NOW();
    if (more && !xt) {   // (with xt the pipeline already holds the next tile's first iterations and its first phase's reads)
      // (the records are requested in front of the barrier, the bases and the first phase's CIGARs behind it)
      const Raw r0 = fetch(nst, wave);
      rawX = fetch(nst, wave + NWAVES);
      nrX = reads_in(nst, wave + NWAVES);
      rawN = fetch_phase(nst, 0, phase_len(wave_its(nst)));
      lds_barrier();       // every tally of this tile is in LDS
      settle(r0, reads_in(nst, wave), bA);
      gather(rawN, ownN);
    } else {
      lds_barrier();       // every tally of this tile is in LDS
    }
    const unsigned long long ps1 = PROBE_NOW();
    uint32_t ticket = 0;
    if (dynamic && take && tid == 0) ticket = atomicAdd(&pe->sched[32 * sched_group], 1u);

    // ---- emit the tile: counts[site][A,C,G,T] (and re-zero LDS), covered / total-depth partials ---------------------------
    MIDAS_MARK("writeout");
    // (a full tile -- all but a contig's last: no row needs a bound, and the LDS reads of four rows are in flight before the first
    // store waits for its own; the overhang sits in the rows below OV only)
    constexpr bool kFullRows = TILE % kDirectBlock == 0 && OUT_IT % 4 == 0;
    const bool full = kFullRows && tile_len == TILE && !(kDebug & (2 | 8));      // workgroup-uniform
    if (full) {
      uint4* const out = reinterpret_cast<uint4*>(pe->out_counts) + tile.site_base;
      uint4* const lds4 = reinterpret_cast<uint4*>(lds);
#pragma unroll
      for (int r0 = 0; r0 < OUT_IT; r0 += 4) {
        uint4 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = lds4[tid + (r0 + r) * kDirectBlock];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = tid + (r0 + r) * kDirectBlock;
          uint4 front = make_uint4(0u, 0u, 0u, 0u);
          if ((r0 + r) * kDirectBlock < OV) {           // (a row the overhang reaches: what this tile's reads added behind it opens the next tile)
            if (cout && i < OV) {
              front = lds4[TILE + i];
              lds4[TILE + i] = make_uint4(0u, 0u, 0u, 0u);
            }
          }
          lds4[i] = front;
          u32x4_a8 nv; nv.x = v[r].x; nv.y = v[r].y; nv.z = v[r].z; nv.w = v[r].w;
          __builtin_nontemporal_store(nv, reinterpret_cast<u32x4_a8*>(out + i));
          const uint32_t d = v[r].x + v[r].y + v[r].z + v[r].w;
          acc_cov += d > 0u ? 1u : 0u;
          acc_depth += d;
        }
      }
    } else {
      uint4* out = reinterpret_cast<uint4*>(pe->out_counts) + ((kDebug & 8) ? 0 : tile.site_base);
      uint4* lds4 = reinterpret_cast<uint4*>(lds);
      const int lim = (kDebug & 2) ? 0 : tile_len;
#pragma unroll
      for (int it = 0; it < OUT_IT; ++it) {
        const int i = tid + it * kDirectBlock;
        if (i < lim) {
          const uint4 v = lds4[i];
          if (cout && i < OV) {                 // what this tile's reads added behind it opens the next tile
            lds4[i] = lds4[TILE + i];
            lds4[TILE + i] = make_uint4(0u, 0u, 0u, 0u);
          } else {
            lds4[i] = make_uint4(0u, 0u, 0u, 0u);
          }
          u32x4_a8 nv; nv.x = v.x; nv.y = v.y; nv.z = v.z; nv.w = v.w;
          __builtin_nontemporal_store(nv, reinterpret_cast<u32x4_a8*>(out + i));
          const uint32_t d = v.x + v.y + v.z + v.w;
          acc_cov += d > 0u ? 1u : 0u;
          acc_depth += d;
        }
      }
    }
    MIDAS_MARK("alleles");
    if (out_allele && full && TILE % (4 * kDirectBlock) == 0) {      // (a full tile: every thread whole words)
      uint8_t* al = out_allele + tile.site_base;
#pragma unroll
      for (int it = 0; it < REF_IT; ++it)
        __builtin_nontemporal_store(upper4(refw[it]), reinterpret_cast<u32_a1*>(al + 4 * (tid + it * kDirectBlock)));
    } else if (out_allele && !(kDebug & 2)) {
      const uint8_t* ref = pe->ref + tile.site_base;
      uint8_t* al = out_allele + tile.site_base;
#pragma unroll
      for (int it = 0; it < REF_IT; ++it) {
        const int i = 4 * (tid + it * kDirectBlock);
        if (i + 4 <= tile_len) {
          __builtin_nontemporal_store(upper4(refw[it]), reinterpret_cast<u32_a1*>(al + i));
        } else {
          for (int j = i; j < tile_len; ++j) {
            uint32_t ch = ref[j];
            if (ch >= 'a' && ch <= 'z') ch -= 32u;
            al[j] = (uint8_t)ch;
          }
        }
      }
    }
    MIDAS_MARK("tiletail");
    if (dynamic && take && tid == 0) s_next_ticket = ticket;
    lds_barrier();       // tallies re-zeroed, this tile's s_stats additions done
#if MIDAS_SNPS_DEBUG_BITS & 256
    pr_sync += ps1 - ps0;
    pr_out += PROBE_NOW() - ps1;
#else
    (void)ps0; (void)ps1;
#endif
    if (take) {
      const long long nn = dynamic ? 2ll * (long long)gridDim.x + (long long)kSchedGroups * s_next_ticket + sched_group
                                   : (long long)i_next + (long long)gridDim.x;
      c_first = item_first(i_next);
      c_end = item_end(i_next);
      i_next = __builtin_amdgcn_readfirstlane((int)(nn < (long long)w_end ? nn : (long long)w_end));
    }
    const bool flush = !more || ntile.species != tile.species;   // workgroup-uniform
    if (flush) {
      for (int d = 32; d >= 1; d >>= 1) {
        acc_cov += __shfl_down(acc_cov, d);
        acc_depth += __shfl_down(acc_depth, d);
      }
      if (lane == 0) {
        if (acc_cov) atomicAdd(&s_stats[MIDAS_STAT_COVERED], (unsigned long long)acc_cov);
        if (acc_depth) atomicAdd(&s_stats[MIDAS_STAT_DEPTH], acc_depth);
      }
      acc_cov = 0u;
      acc_depth = 0ull;
      lds_barrier();
      if (tid < MIDAS_STATS) {
        int ts = tid;
        asm volatile("" : "+v"(ts));      // (formed here: hoisted, the address of this rare add holds two registers through every tile)
        const unsigned long long v = s_stats[ts];
        if (v) atomicAdd(&params_again()->stats[(size_t)tile.species * MIDAS_STATS + ts], v);
        s_stats[ts] = 0ull;
      }
      if (!more) {
        if (dynamic && tid == 0) {   // the last workgroup to leave rewinds the counters for the next launch
          uint32_t* const sched = params_again()->sched;
          if (atomicAdd(&sched[32 * kSchedGroups], 1u) == gridDim.x - 1u) {
            for (int k = 0; k <= kSchedGroups; ++k) sched[32 * k] = 0u;
          }
        }
        break;
      }
      lds_barrier();     // s_stats reset before the next tile adds to it
    }
    t = tn;
    tile = ntile;
    st = nst;
  }
#if MIDAS_SNPS_DEBUG_BITS & 256
  if (lane == 0 && p.probe) {      // per wave: cycles waiting for columns / bases, working, at the barrier, writing out; iterations; all
    unsigned long long* o = p.probe + ((size_t)blockIdx.x * NWAVES + wave) * 8;
    uint32_t hw_id, xcc_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hw_id), "=s"(xcc_id));
    o[0] = pr_cols; o[1] = (unsigned long long)hw_id | ((unsigned long long)xcc_id << 32); o[2] = pr_work; o[3] = pr_sync; o[4] = pr_out; o[5] = pr_iters;
    o[6] = __builtin_readcyclecounter() - pr_t0; o[7] = 0ull;
  }
#endif
#undef PROBE_NOW
}

}  // namespace

int direct_lane_bases(int32_t max_l_seq) {
  // 30 bases per lane: the lanes of a read start 120 tally dwords apart and spread over the LDS banks; 32 only where it
  // saves a whole lane per read (151 bp: 5 lanes instead of 6).  38 (152 dwords apart: the same 24 banks as 30; 40 would be
  // none) where it saves a lane over both: reads of 129 .. 150 bases on four lanes -- 16 of them share a wave-iteration and
  // its per-read instructions, on all 64 lanes, where 30 bases per lane hold 12 on 60 -- and of 97 .. 114 on three.  Shorter
  // reads keep their lanes (not measured), and so do batches of the long overhang (no such instantiation).
  const int l = max_l_seq > 0 ? max_l_seq : 1;
  const int best = (l + 31) / 32 < (l + 29) / 30 ? 32 : 30;
#ifndef MIDAS_DIRECT_NO_LB38
  if (best == 30 && l > 96 && l <= kDirectOverhang && (l + 37) / 38 < (l + 31) / 32) return 38;
#endif
  return best;
}

hipError_t launch_pileup_direct(const DirectParams& p, int lane_bases, hipStream_t stream) {
  if (p.n_tiles <= 0) return hipSuccess;
  const size_t dyn_lds = (size_t)p.table_len * 2 * (p.overhang > kDirectOverhang ? sizeof(int16_t) : sizeof(int32_t));
  const int k = p.chunk_tiles > 1 ? p.chunk_tiles : 1;
  const int n_items = k > 1 ? p.n_chunked_tiles / k + (p.n_tiles - p.n_chunked_tiles) : p.n_tiles;      // (every workgroup of the grid has work)
  const int grid = n_items < p.grid_blocks ? n_items : p.grid_blocks;
  const bool bq0 = p.baseq <= 0;
  if (lane_bases != 30 && lane_bases != 32 && !(lane_bases == 38 && p.overhang <= kDirectOverhang)) return hipErrorInvalidValue;
  if (p.overhang > kDirectOverhang) {      // (a batch of reads longer than the common overhang: the instantiation with the long one)
    if (lane_bases == 32) {
      if (bq0) hipLaunchKernelGGL((pileup_direct_kernel<32, true, kDirectOverhangLong>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
      else hipLaunchKernelGGL((pileup_direct_kernel<32, false, kDirectOverhangLong>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
    } else {
      if (bq0) hipLaunchKernelGGL((pileup_direct_kernel<30, true, kDirectOverhangLong>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
      else hipLaunchKernelGGL((pileup_direct_kernel<30, false, kDirectOverhangLong>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
    }
  } else if (p.lanes_per_read == 4 && p.reads_per_wave == 16) {      // (four lanes per read: the lane geometry is static)
    if (lane_bases == 38) {
      if (bq0) hipLaunchKernelGGL((pileup_direct_kernel<38, true, kDirectOverhang, 4>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
      else hipLaunchKernelGGL((pileup_direct_kernel<38, false, kDirectOverhang, 4>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
    } else if (lane_bases == 32) {
      if (bq0) hipLaunchKernelGGL((pileup_direct_kernel<32, true, kDirectOverhang, 4>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
      else hipLaunchKernelGGL((pileup_direct_kernel<32, false, kDirectOverhang, 4>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
    } else {
      if (bq0) hipLaunchKernelGGL((pileup_direct_kernel<30, true, kDirectOverhang, 4>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
      else hipLaunchKernelGGL((pileup_direct_kernel<30, false, kDirectOverhang, 4>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
    }
  } else if (lane_bases == 38) {
    if (bq0) hipLaunchKernelGGL((pileup_direct_kernel<38, true>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
    else hipLaunchKernelGGL((pileup_direct_kernel<38, false>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
  } else if (lane_bases == 32) {
    if (bq0) hipLaunchKernelGGL((pileup_direct_kernel<32, true>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
    else hipLaunchKernelGGL((pileup_direct_kernel<32, false>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
  } else {
    if (bq0) hipLaunchKernelGGL((pileup_direct_kernel<30, true>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
    else hipLaunchKernelGGL((pileup_direct_kernel<30, false>), dim3(grid), dim3(kDirectBlock), dyn_lds, stream, p);
  }
  return hipGetLastError();
}

}  // namespace midas
