// scan_moments4.hip -- SKEWNESS / KURTOSIS as exact shifted power sums.
//
// The reference folds every doc into a PinotFourthMoment (n, m1, m2, m3, m4) with commons-math's one-pass update
// (FourthMomentAggregationFunction.java, PinotFourthMoment.java): a read-modify-write no atomic table can hold.  Here
// the planner (moments4.cpp) takes a shift K per argument column from the dictionaries' first and last entries and the
// scan accumulates n and the power sums S_k = sum(d^k), k = 1..4, of d = value - K per group: sums that commute.
//
// Integer layouts: K is the column's smallest value over the call's segments, so 0 <= d <= r and every power is
// unsigned.  d^k is split into 32-bit limbs and every limb is added into a 64-bit cell of its own.  A limb is below
// 2^32 and a call holds at most 2^32 docs, so a cell never overflows: every add is a plain no-return 64-bit atomic (or
// a register add in MODE_AGG), nothing carries in the scan, and the cells do not depend on the order of the docs.
//   M4_L8    r < 2^8   d, d^2, d^3, d^4 are one limb each                                  4 cells
//   M4_L16   r < 2^16  d, d^2 one limb; d^3 < 2^48 and d^4 < 2^64 two limbs                6 cells
//   M4_L32   r < 2^32  d one limb, d^2 two, d^3 three (64 x 32 -> 96 bits), d^4 four       10 cells
//   M4_REAL  d = (double) value - K with K the midpoint: d, d^2, d^3, d^4 in four f64 cells, atomicAdd on doubles
// k_moments4_finish reassembles S1..S4 (the only place a carry is propagated), forms the central-moment numerators
// n m2 = n S2 - S1^2, n^2 m3 = n^2 S3 - 3 n S1 S2 + 2 S1^3 and n^3 m4 = n^3 S4 - 4 n^2 S1 S3 + 6 n S1^2 S2 - 3 S1^4
// exactly in 320-bit integers (the largest term, 3 S1^4, is below 2^258), rounds each once to double and divides by
// (double) n k times.
//
// The outer structure is k_scan_moments': workgroups stride over chunks, a workgroup's four waves over a chunk's 64-doc
// words; lane l owns doc 64 w + l.  Per word a wave loads the WHERE clause's mask word (all ones without a bitmap, the
// bits past num_docs cleared) and skips the word when it is zero; a set lane decodes its group key and, per slot, the
// column's dictId and d_of[dictId].
//   MODE_AGG           per-lane cells over the whole chunk loop, a wave reduction by shuffles, the four waves combined
//                      in LDS, one atomic per workgroup, slot and cell
//   MODE_GROUP_LDS     per-workgroup tables in LDS -- n[G], then per slot its cells, [G] each -- flushed to the HBM
//                      tables at the end (zero cells are skipped)
//   MODE_GROUP_GLOBAL  the same adds, straight into the HBM tables
// A limb that is zero issues no atomic.  The docs matched per segment (wave-uniform popcounts, one atomic per chunk and
// wave) give the statistics.
#include <algorithm>

#include "limbs_to_double.h"
#include "scan_kernel.h"

namespace ph {

typedef const PH_CONST MSegment* M4SegPtr;
typedef unsigned long long u64;

__device__ __forceinline__ double m4_f64(u64 b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ u64 m4_bits(double x) { return (u64)__double_as_longlong(x); }

// the cells one doc adds to a slot, from its d_of entry
template <int L>
__device__ __forceinline__ void m4_term(long long dv, u64 (&t)[m4_cells(L)]) {
  constexpr u64 M = 0xffffffffull;
  if constexpr (L == M4_REAL) {
    const double x = __longlong_as_double(dv), x2 = x * x;
    t[0] = m4_bits(x);
    t[1] = m4_bits(x2);
    t[2] = m4_bits(x2 * x);
    t[3] = m4_bits(x2 * x2);
  } else if constexpr (L == M4_L8) {
    const uint32_t d = (uint32_t)dv, d2 = d * d;  // d <= 255: d^4 < 2^32
    t[0] = d;
    t[1] = d2;
    t[2] = d2 * d;
    t[3] = d2 * d2;
  } else if constexpr (L == M4_L16) {
    const uint32_t d = (uint32_t)dv, d2 = d * d;  // d < 2^16: d^2 < 2^32
    const u64 d3 = (u64)d2 * d, d4 = (u64)d2 * d2;
    t[0] = d;
    t[1] = d2;
    t[2] = d3 & M;
    t[3] = d3 >> 32;
    t[4] = d4 & M;
    t[5] = d4 >> 32;
  } else {
    const u64 d = (u64)dv, d2 = d * d;  // d < 2^32: d^2 < 2^64, d^3 < 2^96, d^4 < 2^128
    const u64 d3lo = d2 * d, d3hi = __umul64hi(d2, d), d4lo = d2 * d2, d4hi = __umul64hi(d2, d2);
    t[0] = d;
    t[1] = d2 & M;
    t[2] = d2 >> 32;
    t[3] = d3lo & M;
    t[4] = d3lo >> 32;
    t[5] = d3hi;
    t[6] = d4lo & M;
    t[7] = d4lo >> 32;
    t[8] = d4hi & M;
    t[9] = d4hi >> 32;
  }
}

// a += b in registers
template <int L>
__device__ __forceinline__ void m4_add(u64& a, u64 b) {
  if constexpr (L == M4_REAL) a = m4_bits(m4_f64(a) + m4_f64(b));
  else a += b;
}

// *cell += v, result unused: a no-return atomic on an LDS or an HBM cell alike
template <int L>
__device__ __forceinline__ void m4_atomic(u64* cell, u64 v) {
  if constexpr (L == M4_REAL) atomicAdd(reinterpret_cast<double*>(cell), m4_f64(v));
  else atomicAdd(cell, v);
}

constexpr int kM4AggCells = 1 + kMMaxSlots * kM4MaxCells;  // MODE_AGG: n and the slots' cells per wave in LDS

template <int MODE, int L>
__global__ void __launch_bounds__(kBlock) k_scan_moments4(const M4Params p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char m4_lds[];
  u64* lds = reinterpret_cast<u64*>(m4_lds);
  constexpr int NC = m4_cells(L);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ns = p.num_slots;
  const int64_t G = p.num_groups;
  const bool counting = p.n != nullptr;

  if (MODE == MODE_GROUP_LDS) {
    for (int64_t i = threadIdx.x; i < (int64_t)(1 + ns * NC) * G; i += kBlock) lds[i] = 0ull;  // (+0.0 too)
    __syncthreads();
  }

  u64 an = 0ull;
  u64 acc[MODE == MODE_AGG ? kMMaxSlots : 1][NC];
#pragma unroll
  for (int s = 0; s < (MODE == MODE_AGG ? kMMaxSlots : 1); ++s)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[s][c] = 0ull;

  for (int c = p.chunk_begin + (int)blockIdx.x; c < p.chunk_end; c += (int)gridDim.x) {
    const PH_CONST Chunk* ck = (const PH_CONST Chunk*)p.chunks + c;  // C-style cast = addrspacecast
    const int32_t seg = ck->seg, wb = ck->word_begin, we = ck->word_end;
    M4SegPtr S = (M4SegPtr)p.segs + seg;
    const int32_t nd = S->num_docs;
    const u64* mask = S->mask;
    u64 pc = 0ull;  // wave-uniform: this wave's matched docs of the chunk
    for (int32_t w = wb + wave; w < we; w += kWaves) {
      const int32_t left = nd - w * 64;
      if (left <= 0) break;
      u64 m = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
      if (mask) m &= gld(mask + w);
      if (m == 0ull) continue;
      pc += (u64)__popcll(m);
      if (!((m >> lane) & 1ull)) continue;
      const uint32_t doc = (uint32_t)w * 64u + (uint32_t)lane;
      int64_t key = 0;
      if (MODE != MODE_AGG) {
#pragma unroll
        for (int g = 0; g < kMaxGroupCols; ++g) {
          if (g < p.num_group_cols) {
            uint32_t id = unpack_bits(S->gfwd[g], S->gbits[g], doc);
            const int32_t* rm = S->gremap[g];
            if (rm) id = (uint32_t)gld(rm + id);
            key += (int64_t)id * p.group_stride[g];
          }
        }
        if (key < 0 || key >= G) continue;  // (never: remapped ids index the call's dictionaries)
        if (counting) {
          if (MODE == MODE_GROUP_LDS) atomicAdd(lds + key, 1ull);
          else atomicAdd(p.n + key, 1ull);
        }
      } else {
        an += 1ull;
      }
#pragma unroll
      for (int s = 0; s < kMMaxSlots; ++s) {
        if (s < ns) {
          const int v = p.slot_col[s];
          const uint32_t id = unpack_bits(S->vfwd[v], S->vbits[v], doc);
          u64 t[NC];
          m4_term<L>(gld(S->d_of[v] + id), t);
          if constexpr (MODE == MODE_AGG) {
#pragma unroll
            for (int k = 0; k < NC; ++k) m4_add<L>(acc[s][k], t[k]);
          } else {
            u64* base = MODE == MODE_GROUP_LDS ? lds + (int64_t)(1 + s * NC) * G + key : p.cells[s] + key;
#pragma unroll
            for (int k = 0; k < NC; ++k)
              if (t[k]) m4_atomic<L>(base + (int64_t)k * G, t[k]);
          }
        }
      }
    }
    if (counting && lane == 0 && pc) atomicAdd(p.seg_count + seg, pc);
  }

  if constexpr (MODE == MODE_AGG) {
    // wave reductions by shuffles (limb sums stay below 2^64 over the whole call, so they add as plain u64), the
    // workgroup's waves combined in LDS, one atomic per workgroup, slot and cell
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) an += (u64)__shfl_xor((long long)an, o, 64);
    if (lane == 0) lds[wave * kM4AggCells] = an;
#pragma unroll
    for (int s = 0; s < kMMaxSlots; ++s) {
      if (s < ns) {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          u64 v = acc[s][k];
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) m4_add<L>(v, (u64)__shfl_xor((long long)v, o, 64));
          if (lane == 0) lds[wave * kM4AggCells + 1 + s * NC + k] = v;
        }
      }
    }
    __syncthreads();
    u64 docs = 0ull;
    for (int k = 0; k < kWaves; ++k) docs += lds[k * kM4AggCells];
    if (docs && (int)threadIdx.x < ns * NC) {
      const int s = (int)threadIdx.x / NC, k = (int)threadIdx.x - s * NC;
      u64 v = 0ull;
      for (int wv = 0; wv < kWaves; ++wv) m4_add<L>(v, lds[wv * kM4AggCells + 1 + s * NC + k]);
      u64* dst = nullptr;  // (a static index into the by-value parameter array)
#pragma unroll
      for (int j = 0; j < kMMaxSlots; ++j)
        if (j == s) dst = p.cells[j];
      if (v) m4_atomic<L>(dst + (int64_t)k * G, v);
    }
    if (docs && threadIdx.x == 0 && counting) atomicAdd(p.n, docs);
  } else if constexpr (MODE == MODE_GROUP_LDS) {
    __syncthreads();
    for (int64_t g = threadIdx.x; g < G; g += kBlock) {
      const u64 docs = lds[g];  // (0 everywhere in a launch that does not count)
      if (docs) atomicAdd(p.n + g, docs);
#pragma unroll
      for (int s = 0; s < kMMaxSlots; ++s) {
        if (s < ns) {
#pragma unroll
          for (int k = 0; k < NC; ++k) {
            const u64 v = lds[(int64_t)(1 + s * NC + k) * G + g];
            if (v) m4_atomic<L>(p.cells[s] + (int64_t)k * G + g, v);
          }
        }
      }
    }
  }
}

// ---- finish: (n, cells) -> PinotFourthMoment

// a 320-bit unsigned integer, w[0] lowest; every loop below is unrolled, so the words stay in registers
struct W5 {
  u64 w[5];
};

__device__ __forceinline__ W5 w_of(u64 x) { return W5{{x, 0ull, 0ull, 0ull, 0ull}}; }

// a += v << (32 J): where a limb cell, itself up to 64 bits, lands in its power sum
template <int J>
__device__ __forceinline__ void w_add_limb(W5& a, u64 v) {
  constexpr int at = J >> 1;
  u64 add[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
  if constexpr (J & 1) {
    add[at] = v << 32;
    add[at + 1] = v >> 32;
  } else {
    add[at] = v;
  }
  u64 carry = 0ull;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const u64 s1 = a.w[k] + add[k], c1 = s1 < add[k] ? 1ull : 0ull;
    const u64 s2 = s1 + carry, c2 = s2 < carry ? 1ull : 0ull;
    a.w[k] = s2;
    carry = c1 | c2;
  }
}

__device__ __forceinline__ void w_add(W5& a, const W5& b) {
  u64 carry = 0ull;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const u64 s1 = a.w[k] + b.w[k], c1 = s1 < b.w[k] ? 1ull : 0ull;
    const u64 s2 = s1 + carry, c2 = s2 < carry ? 1ull : 0ull;
    a.w[k] = s2;
    carry = c1 | c2;
  }
}

// a x b, the low 320 bits (the callers' products stay below 2^260)
__device__ __forceinline__ W5 w_mul(const W5& a, u64 b) {
  W5 r;
  u64 carry = 0ull;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const u64 lo = a.w[k] * b, hi = __umul64hi(a.w[k], b);
    r.w[k] = lo + carry;
    carry = hi + (r.w[k] < lo ? 1ull : 0ull);  // (hi <= 2^64 - 2: no overflow)
  }
  return r;
}

// (a - b) as a double: the magnitude of the exact difference rounded once to nearest-even
__device__ __forceinline__ double w_diff_to_double(W5 a, const W5& b) {
  u64 borrow = 0ull;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const u64 d1 = a.w[k] - b.w[k], b1 = a.w[k] < b.w[k] ? 1ull : 0ull;
    const u64 d2 = d1 - borrow, b2 = d1 < borrow ? 1ull : 0ull;
    a.w[k] = d2;
    borrow = b1 | b2;
  }
  const bool neg = borrow != 0ull;
  if (neg) {  // two's complement of the wrapped difference
    u64 carry = 1ull;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      a.w[k] = ~a.w[k] + carry;
      carry = (carry && a.w[k] == 0ull) ? 1ull : 0ull;
    }
  }
  const double d = m_limbs_to_double(a.w);
  return neg ? -d : d;
}

// S1..S4 of one (group, slot) from its limb cells: here, once, the carries are propagated
template <int L>
__device__ __forceinline__ void m4_assemble(const u64* cells, int64_t G, int64_t g, u64& s1, W5& s2, W5& s3, W5& s4) {
  u64 c[m4_cells(L)];
#pragma unroll
  for (int k = 0; k < m4_cells(L); ++k) c[k] = gld(cells + (int64_t)k * G + g);
  s1 = c[0];  // (< 2^64: d < 2^32 and at most 2^32 docs)
  if constexpr (L == M4_L8) {
    s2 = w_of(c[1]);
    s3 = w_of(c[2]);
    s4 = w_of(c[3]);
  } else if constexpr (L == M4_L16) {
    s2 = w_of(c[1]);
    s3 = w_of(c[2]);
    w_add_limb<1>(s3, c[3]);
    s4 = w_of(c[4]);
    w_add_limb<1>(s4, c[5]);
  } else {
    s2 = w_of(c[1]);
    w_add_limb<1>(s2, c[2]);
    s3 = w_of(c[3]);
    w_add_limb<1>(s3, c[4]);
    w_add_limb<2>(s3, c[5]);
    s4 = w_of(c[6]);
    w_add_limb<1>(s4, c[7]);
    w_add_limb<2>(s4, c[8]);
    w_add_limb<3>(s4, c[9]);
  }
}

__global__ void __launch_bounds__(256) k_moments4_finish(const M4FinishParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.num_groups * p.num_slots) return;
  const int sl = (int)(i / p.num_groups);
  const int64_t G = p.num_groups, g = i - (int64_t)sl * G;
  // (static indices into the by-value parameter arrays: a dynamic one would copy them to scratch)
  int layout = 0;
  long long K = 0;
  const u64* cells = nullptr;
  M4Tuple* dst = nullptr;
#pragma unroll
  for (int k = 0; k < kMMaxSlots; ++k)
    if (k == sl) {
      layout = p.layout[k];
      K = p.shift[k];
      cells = p.cells[k];
      dst = p.out[k];
    }
  const u64 n = gld(p.n + g);
  // no doc: commons-math's FourthMoment() leaves m1..m4 NaN
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  M4Tuple out{(int64_t)n, nan, nan, nan, nan};
  if (n) {
    const double dn = (double)n;
    if (layout == M4_REAL) {
      const double k = __longlong_as_double(K);
      const double s1 = m4_f64(gld(cells + g)), s2 = m4_f64(gld(cells + G + g)), s3 = m4_f64(gld(cells + 2 * G + g)),
                   s4 = m4_f64(gld(cells + 3 * G + g));
      const double a = s1 / dn;  // the mean of d
      out.m1 = k + a;
      out.m2 = fmax(0.0, s2 - s1 * a);
      out.m3 = s3 - 3.0 * a * s2 + 2.0 * a * a * s1;
      out.m4 = fmax(0.0, s4 - 4.0 * a * s3 + 6.0 * a * a * s2 - 3.0 * a * a * a * s1);
    } else {
      u64 s1;
      W5 s2, s3, s4;
      if (layout == M4_L8) m4_assemble<M4_L8>(cells, G, g, s1, s2, s3, s4);
      else if (layout == M4_L16) m4_assemble<M4_L16>(cells, G, g, s1, s2, s3, s4);
      else m4_assemble<M4_L32>(cells, G, g, s1, s2, s3, s4);
      // m1 = (n K + S1) / n: the exact integer rounded once, one division
      W5 nk = w_mul(w_of(n), K < 0 ? 0ull - (u64)K : (u64)K);  // n |K|
      if (K < 0) {
        out.m1 = w_diff_to_double(w_of(s1), nk) / dn;
      } else {
        w_add(nk, w_of(s1));
        out.m1 = m_limbs_to_double(nk.w) / dn;
      }
      // n m2 = n S2 - S1^2 (>= 0 by Cauchy-Schwarz)
      const W5 q1 = w_of(s1), q2 = w_mul(q1, s1), q3 = w_mul(q2, s1), q4 = w_mul(q3, s1);  // S1^k
      out.m2 = w_diff_to_double(w_mul(s2, n), q2) / dn;
      // n^2 m3 = (n^2 S3 + 2 S1^3) - 3 n S1 S2 (signed)
      W5 pos = w_mul(w_mul(s3, n), n);
      w_add(pos, w_mul(q3, 2ull));
      out.m3 = w_diff_to_double(pos, w_mul(w_mul(w_mul(s2, s1), n), 3ull)) / dn / dn;
      // n^3 m4 = (n^3 S4 + 6 n S1^2 S2) - (4 n^2 S1 S3 + 3 S1^4) (>= 0)
      pos = w_mul(w_mul(w_mul(s4, n), n), n);
      w_add(pos, w_mul(w_mul(w_mul(w_mul(s2, s1), s1), n), 6ull));
      W5 sub = w_mul(w_mul(w_mul(w_mul(s3, s1), n), n), 4ull);
      w_add(sub, w_mul(q4, 3ull));
      out.m4 = w_diff_to_double(pos, sub) / dn / dn / dn;
    }
  }
  dst[g] = out;
}

size_t moments4_lds_bytes(const M4Params& p, int mode, int layout) {
  if (mode == MODE_AGG) return (size_t)kWaves * kM4AggCells * 8;
  if (mode == MODE_GROUP_LDS) return (size_t)(1 + p.num_slots * m4_cells(layout)) * (size_t)p.num_groups * 8;
  return 0;
}

template <int MODE, int L>
static void launch_layout(const M4Params& p, int grid, size_t lds, hipStream_t s) {
  allow_lds(k_scan_moments4<MODE, L>, lds);
  hipLaunchKernelGGL((k_scan_moments4<MODE, L>), dim3(grid), dim3(kBlock), lds, s, p);
}

template <int MODE>
static void launch_mode(const M4Params& p, int layout, int grid, size_t lds, hipStream_t s) {
  switch (layout) {
    case M4_L8: launch_layout<MODE, M4_L8>(p, grid, lds, s); break;
    case M4_L16: launch_layout<MODE, M4_L16>(p, grid, lds, s); break;
    case M4_L32: launch_layout<MODE, M4_L32>(p, grid, lds, s); break;
    case M4_REAL: launch_layout<MODE, M4_REAL>(p, grid, lds, s); break;
    default: fail(PH_ERR_INVALID_ARGUMENT, "fourth-moment scan with a bad layout");
  }
}

void launch_scan_moments4(const M4Params& p, int mode, int layout, int grid, hipStream_t s) {
  if (!p.segs || !p.chunks || p.num_slots <= 0 || p.num_slots > kMMaxSlots || p.num_group_cols < 0 ||
      p.num_group_cols > kMaxGroupCols || p.num_groups <= 0 || (p.n == nullptr) != (p.seg_count == nullptr) ||
      grid <= 0)
    fail(PH_ERR_INVALID_ARGUMENT, "fourth-moment scan with bad parameters");
  for (int i = 0; i < p.num_slots; ++i)
    if (!p.cells[i] || p.slot_col[i] < 0 || p.slot_col[i] >= kMMaxSlots)
      fail(PH_ERR_INVALID_ARGUMENT, "fourth-moment scan with a bad slot");
  const size_t lds = moments4_lds_bytes(p, mode, layout);
  if (lds > 160 * 1024) fail(PH_ERR_INVALID_ARGUMENT, "fourth-moment scan tables exceed the LDS of one CU");
  switch (mode) {
    case MODE_AGG: launch_mode<MODE_AGG>(p, layout, grid, lds, s); break;
    case MODE_GROUP_LDS: launch_mode<MODE_GROUP_LDS>(p, layout, grid, lds, s); break;
    case MODE_GROUP_GLOBAL: launch_mode<MODE_GROUP_GLOBAL>(p, layout, grid, lds, s); break;
    default: fail(PH_ERR_UNSUPPORTED, "fourth moments in this plan mode");
  }
  PH_HIP_CHECK(hipGetLastError());
}

void launch_moments4_finish(const M4FinishParams& p, hipStream_t s) {
  if (p.num_groups <= 0 || p.num_slots <= 0 || p.num_slots > kMMaxSlots || !p.n)
    fail(PH_ERR_INVALID_ARGUMENT, "fourth-moment finish with bad parameters");
  const int64_t threads = p.num_groups * p.num_slots;
  hipLaunchKernelGGL(k_moments4_finish, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, p);
  PH_HIP_CHECK(hipGetLastError());
}

}  // namespace ph
