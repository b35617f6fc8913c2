// The kernels of a two-group permutation test over rows of values (gene_assoc.py), kept apart from the gene
// matrix so that a later command over other rows can include them: the relabellings expanded to bytes, the doubled midranks of
// the kept rows as 7-bit digits, and the product of the digits with the relabellings that counts the relabellings at least as
// extreme as the case labelling.  Everything is integer but the comparisons of the parsed doubles (<, ==, > cutoff): nothing
// here depends on -ffp-contract.  Everything has internal linkage.
//
// The axes.  The N used samples are numbered j = 0 .. N-1 in column order (col_of[j] = the column, is_case[j] = 1 for a case);
// Kp = N rounded up to 64, the K step of v_mfma_i32_16x16x64_i8; the bytes j >= N of every image are 0.
//   relabellings   img [Ppad][Kp] int8: img[b][j] = bit col_of[j] of plane b; Ppad = P rounded up to 16, the rows b >= P are 0
//   digits         lo, hi [rows of the group][Kp] int8, a kept row at its place among the group's kept rows: r & 127 and r >> 7 of
//                  the doubled midrank r (2 .. 2N <= 16 382 = 127 * 128 + 126: both digits are non-negative signed bytes); under
//                  presabs lo is the 0 / 1 presence and there is no hi
//   product        s(b) = sum over j of r_j * img[b][j], accumulated in i32 (at most 127 * 8 191 a digit), hi * 128 + lo
// The MFMA operands.  v_mfma_i32_16x16x64_i8 takes 16 bytes of A and of B a lane: lane l holds A[row l & 15][k] and
// B[k][column l & 15] for the 16 values of k that belong to l >> 4, and D[row 4 (l >> 4) + reg][column l & 15] in its four
// accumulators.  Both operands here are K-contiguous images read with the same address rule, ks * 64 + 16 (l >> 4) + byte, so a
// byte of A always meets the byte of B of the same sample, whichever k the hardware gives the pair: the sum over k does not
// depend on it.  What the kernel relies on is the row / column on l & 15 and the D map; the identity test
// (tests/test_gpu_gene_assoc.py) holds both to exact integers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace midas {
namespace {

typedef int as_v4i __attribute__((ext_vector_type(4)));

constexpr int kAsTile = 32;          // kept rows a workgroup of the product kernel owns: two 16-row tiles
constexpr int kAsMaxUsed = 8191;     // used samples: 2 N must fit two 7-bit digits
constexpr int kAsLdsBytes = 60 * 1024;      // the digits of a tile lie in LDS while they fit this

// a thread four bytes of the image
__global__ __launch_bounds__(256) void as_expand_kernel(const unsigned long long* planes, int W, const int32_t* col_of, int N, int Kp,
                                                        long long P, long long Ppad, int8_t* img) {
  const long long at = (long long)blockIdx.x * 256 + threadIdx.x, per = Kp / 4;
  if (at >= Ppad * per) return;
  const long long b = at / per;
  const int j0 = (int)(at - b * per) * 4;
  uint32_t v = 0;
  if (b < P)
    for (int i = 0; i < 4; ++i) {
      const int j = j0 + i;
      if (j >= N) break;
      const int c = col_of[j];
      v |= (uint32_t)((planes[b * W + (c >> 6)] >> (c & 63)) & 1ull) << (8 * i);
    }
  reinterpret_cast<uint32_t*>(img)[at] = v;
}

struct AsRankP {
  const double* val;            // [columns][stride]: the group's cells
  long long stride;
  const int32_t* col_of;        // [N]
  const uint8_t* is_case;       // [N]
  int N, Kp, R;                 // R: rows a workgroup (a power of two, R * N <= kAsMaxUsed, at most 64)
  double cutoff;
  const uint32_t *flag, *rank;  // [g] the row is kept; the kept rows before it in the group
  const int32_t *c, *a;         // [g] presence count and presence count among the cases
  long long g, base_row, k0, room;      // rows of the group; its first row; slots before the group; entries of the slot arrays
  int8_t *lo, *hi;              // the group's digits
  int32_t *row_of_slot, *count, *count_case;      // [room]
  unsigned long long *w, *ties; // [room], zero before the call: sum of r over the cases; sum of e^2 - 1
};

// kKind 0: r = presence; 1: r = the doubled midrank 2 #{t: v_t < v_s} + #{t: v_t == v_s} + 1 over the N used samples, by counting.
// The R rows' used values lie in LDS; 256 / R threads share a row, a thread every (256 / R)-th sample of it.
template <int kKind>
__global__ __launch_bounds__(256) void as_rank_kernel(AsRankP p) {
  __shared__ double s_v[kAsMaxUsed];
  const int R = p.R, tpr = 256 / R, N = p.N, Kp = p.Kp;
  const long long row0 = (long long)blockIdx.x * R;
  for (int e = threadIdx.x; e < R * N; e += 256) {
    const int i = e % R, j = e / R;
    const long long r = row0 + i;
    s_v[i * N + j] = r < p.g ? p.val[(long long)p.col_of[j] * p.stride + r] : 0.0;
  }
  __syncthreads();
  const int i = threadIdx.x / tpr, q = threadIdx.x % tpr;
  const long long r = row0 + i;
  const bool kept = r < p.g && p.flag[r] != 0u;
  const long long gs = kept ? (long long)p.rank[r] : 0;
  long long w = 0, t = 0;
  if (kept) {
    const double* v = s_v + i * N;
    int8_t* lo = p.lo + gs * Kp;
    int8_t* hi = kKind ? p.hi + gs * Kp : nullptr;
    for (int s = q; s < Kp; s += tpr) {
      int rk = 0;
      if (s < N) {
        const double x = v[s];
        if (kKind == 0) {
          rk = x > p.cutoff ? 1 : 0;
        } else {
          int lt = 0, eq = 0;
          for (int u = 0; u < N; ++u) {
            const double y = v[u];
            lt += y < x ? 1 : 0;
            eq += y == x ? 1 : 0;
          }
          rk = 2 * lt + eq + 1;
          t += (long long)eq * eq - 1;
        }
        if (p.is_case[s]) w += rk;
      }
      lo[s] = (int8_t)(rk & 127);
      if (kKind) hi[s] = (int8_t)(rk >> 7);
    }
  }
  // (every lane: the partners of a lane share its row, so they are kept or dropped together)
  for (int o = (tpr < 64 ? tpr : 64) / 2; o > 0; o >>= 1) {
    w += __shfl_xor(w, o);
    t += __shfl_xor(t, o);
  }
  const long long slot = p.k0 + gs;
  if (!kept || slot >= p.room || (q & 63) != 0) return;
  atomicAdd(&p.w[slot], (unsigned long long)w);       // (integer sums: any order gives the same bits)
  atomicAdd(&p.ties[slot], (unsigned long long)t);
  if (q == 0) {
    p.row_of_slot[slot] = (int32_t)(p.base_row + r);
    p.count[slot] = p.c[r];
    p.count_case[slot] = p.a[r];
  }
}

struct AsProdP {
  const int8_t *lo, *hi;        // the group's digits, [kept rows of the group][Kp]
  const int8_t* img;            // [Ppad][Kp]
  const unsigned long long* planes;     // [P][W]: the walk kernel reads the bits themselves
  const int32_t* col_of;
  int W, Kp, N, n1;
  long long P;
  const uint32_t *last_flag, *last_rank;        // their sum = the kept rows of the group
  long long k0, room;
  const int32_t* count;         // [room]
  const unsigned long long* w;  // [room]
  uint32_t* exceed;             // [room]
  int32_t* products;            // null, or [prod_cap]: slot * P + b
  long long prod_cap;
};

// |x(M_b)| >= |x(L0)| with x = N a - n1 c under presabs and w - n1 (N + 1) under copynum: base and thr a row, the factor by kind
__device__ __forceinline__ void as_row_constants(const AsProdP& p, bool presabs, long long slot, int* base, int* thr) {
  const int w0 = (int)p.w[slot];
  *base = presabs ? p.n1 * p.count[slot] : p.n1 * (p.N + 1);
  const int x0 = (presabs ? p.N * w0 : w0) - *base;
  *thr = x0 < 0 ? -x0 : x0;
}

// Form 1.  A workgroup owns kAsTile kept rows over every relabelling; wave v takes the 16-relabelling tiles v, v + 4, ...: for each
// it walks K in steps of 64 with one B fragment from the image and, per 16-row tile and digit, one A fragment from LDS (kLds) or
// from memory, recombines the digits, writes the product where it is asked for and compares on the accumulators.  The counts of
// a row meet by lane exchange and through LDS: no atomics.  kDigits == 1 is presabs.
template <int kDigits, bool kLds>
__global__ __launch_bounds__(256) void as_product_kernel(AsProdP p) {
  extern __shared__ __align__(16) int8_t s_a[];         // kLds: [kDigits][kAsTile][Kp + 16]
  __shared__ int s_base[kAsTile], s_thr[kAsTile];
  __shared__ uint32_t s_cnt[4][kAsTile];
  const long long kg = (long long)*p.last_flag + (long long)*p.last_rank, t0 = (long long)blockIdx.x * kAsTile;
  if (t0 >= kg) return;                                 // (the whole workgroup)
  const int n_g = kg - t0 < kAsTile ? (int)(kg - t0) : kAsTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, Kp = p.Kp, ld = Kp + 16, per = Kp / 16;
  const int li = lane & 15, lh = lane >> 4;
  if (kLds) {
    for (int e = tid; e < kDigits * kAsTile * per; e += 256) {
      const int d = e / (kAsTile * per), rem = e - d * kAsTile * per, i = rem / per, c = rem - i * per;
      as_v4i x = {0, 0, 0, 0};
      if (i < n_g) x = *reinterpret_cast<const as_v4i*>((d ? p.hi : p.lo) + (t0 + i) * Kp + c * 16);
      *reinterpret_cast<as_v4i*>(s_a + (d * kAsTile + i) * ld + c * 16) = x;
    }
  }
  if (tid < kAsTile) {
    int base = 0, thr = 0;
    if (tid < n_g) as_row_constants(p, kDigits == 1, p.k0 + t0 + tid, &base, &thr);
    s_base[tid] = base;
    s_thr[tid] = thr;
  }
  __syncthreads();
  const int mul = kDigits == 1 ? p.N : 1;
  uint32_t cnt[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  const long long tiles = (p.P + 15) / 16;
  for (long long pt = wave; pt < tiles; pt += 4) {
    as_v4i acc[2][kDigits];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int d = 0; d < kDigits; ++d) acc[m][d] = as_v4i{0, 0, 0, 0};
    const int8_t* brow = p.img + (pt * 16 + li) * Kp + 16 * lh;
    for (int ks = 0; ks < Kp; ks += 64) {
      const as_v4i b = *reinterpret_cast<const as_v4i*>(brow + ks);
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int d = 0; d < kDigits; ++d) {
          const int i = m * 16 + li;
          as_v4i a = {0, 0, 0, 0};
          if (kLds) a = *reinterpret_cast<const as_v4i*>(s_a + (d * kAsTile + i) * ld + ks + 16 * lh);
          else if (i < n_g) a = *reinterpret_cast<const as_v4i*>((d ? p.hi : p.lo) + (t0 + i) * Kp + ks + 16 * lh);
          acc[m][d] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[m][d], 0, 0, 0);
        }
    }
    const long long perm = pt * 16 + li;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int i = m * 16 + lh * 4 + reg;
        const int s = kDigits == 1 ? acc[m][0][reg] : acc[m][kDigits - 1][reg] * 128 + acc[m][0][reg];
        if (perm >= p.P || i >= n_g) continue;
        const long long at = (p.k0 + t0 + i) * p.P + perm;
        if (p.products && at < p.prod_cap) p.products[at] = s;
        const int x = mul * s - s_base[i];
        cnt[m][reg] += (x < 0 ? -x : x) >= s_thr[i] ? 1u : 0u;
      }
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      uint32_t n = cnt[m][reg];
      for (int o = 8; o > 0; o >>= 1) n += __shfl_xor(n, o);
      if (li == 0) s_cnt[wave][m * 16 + lh * 4 + reg] = n;
    }
  __syncthreads();
  if (tid < n_g && p.k0 + t0 + tid < p.room) p.exceed[p.k0 + t0 + tid] = s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
}

// Form 0, the cross-check: a thread a (kept row, relabelling) walks the used samples, reads the sample's bit from the plane
// itself and adds the rank with plain integer adds; the hits of a row meet by atomicAdd (exceed is zero before the call).
__global__ __launch_bounds__(256) void as_walk_kernel(AsProdP p, int presabs) {
  const long long kg = (long long)*p.last_flag + (long long)*p.last_rank, n = kg * p.P;
  for (long long at = (long long)blockIdx.x * 256 + threadIdx.x; at < n; at += (long long)gridDim.x * 256) {
    const long long gs = at / p.P, b = at - gs * p.P, slot = p.k0 + gs;
    if (slot >= p.room) continue;
    const int8_t *lo = p.lo + gs * p.Kp, *hi = presabs ? nullptr : p.hi + gs * p.Kp;
    const unsigned long long* plane = p.planes + b * p.W;
    int s = 0;
    for (int j = 0; j < p.N; ++j) {
      const int c = p.col_of[j];
      if ((plane[c >> 6] >> (c & 63)) & 1ull) s += presabs ? (int)lo[j] : (int)hi[j] * 128 + (int)lo[j];
    }
    const long long pa = slot * p.P + b;
    if (p.products && pa < p.prod_cap) p.products[pa] = s;
    int base, thr;
    as_row_constants(p, presabs != 0, slot, &base, &thr);
    const int x = (presabs ? p.N : 1) * s - base;
    if ((x < 0 ? -x : x) >= thr) atomicAdd(&p.exceed[slot], 1u);
  }
}

}  // namespace
}  // namespace midas
