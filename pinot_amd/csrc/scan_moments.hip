// scan_moments.hip -- the variance family (VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP) as exact shifted moments.
//
// The reference folds every doc into a (count, sum, m2) tuple with Chan's update (VarianceAggregationFunction.java:
// 80-121, VarianceTuple.apply :35-44): a read-modify-write no atomic table can hold.  Here the planner (moments.cpp)
// takes a shift K per argument column from the dictionaries' first and last entries, so d = value - K is small, and the
// scan accumulates n, S1 = sum(d) and S2 = sum(d^2) per group: sums that commute, exact integers in the integer forms.
// k_moments_finish turns them into the reference's tuple: sum = n K + S1, m2 = (n S2 - S1^2) / n.
//
// Workgroups stride over chunks, a workgroup's four waves over a chunk's 64-doc words; lane l owns doc 64 w + l.  Per
// word a wave loads the WHERE clause's mask word (all ones without a bitmap, the bits past num_docs cleared) and skips
// the word when it is zero; a set lane decodes its group key and, per slot, the column's dictId and d_of[dictId].
//   MODE_AGG           per-lane (n, S1, S2) over the whole chunk loop, a wave reduction by shuffles, the four waves
//                      combined in LDS, one set of atomics per workgroup per slot
//   MODE_GROUP_LDS     per-workgroup tables in LDS -- n[G], then per slot S1[G], S2lo[G] and (wide) S2hi[G] -- flushed
//                      to the HBM tables at the end (groups the workgroup saw no doc of are skipped)
//   MODE_GROUP_GLOBAL  the same adds, straight into the HBM tables
//   MFORM_NARROW       S2 is one u64 (the planner's bound: it never carries): no-return atomics only
//   MFORM_WIDE         d^2 is a 64 x 64 -> 128 product added into a (lo, hi) pair; in a table the add of the low half
//                      returns the old value, and the carry it shows goes into the high half with the product's own
//   MFORM_REAL         doubles, atomicAdd on doubles
// The docs matched per segment (wave-uniform popcounts, one atomic per chunk and wave) give the statistics.
#include <algorithm>

#include "limbs_to_double.h"
#include "scan_kernel.h"

namespace ph {

typedef const PH_CONST MSegment* MSegPtr;
typedef unsigned long long u64;

// the three cells one doc (or one partial sum) adds to a slot: S1, and S2 as (lo, hi); doubles' bits in MFORM_REAL
struct MTerm {
  u64 s1, lo, hi;
};

template <int FORM>
__device__ __forceinline__ MTerm m_term(long long d) {
  MTerm t;
  t.s1 = (u64)d;
  t.hi = 0ull;
  if (FORM == MFORM_REAL) {
    const double x = __longlong_as_double(d);
    t.lo = (u64)__double_as_longlong(x * x);
  } else if (FORM == MFORM_NARROW) {
    t.lo = (u64)d * (u64)d;  // d^2 < 2^64 by the planner's bound, so the low product is all of it
  } else {
    const u64 a = d < 0 ? 0ull - (u64)d : (u64)d;
    t.lo = a * a;
    t.hi = __umul64hi(a, a);
  }
  return t;
}

// a += b in registers
template <int FORM>
__device__ __forceinline__ void m_combine(MTerm& a, const MTerm& b) {
  if (FORM == MFORM_REAL) {
    a.s1 = (u64)__double_as_longlong(__longlong_as_double((long long)a.s1) + __longlong_as_double((long long)b.s1));
    a.lo = (u64)__double_as_longlong(__longlong_as_double((long long)a.lo) + __longlong_as_double((long long)b.lo));
  } else {
    a.s1 += b.s1;
    a.lo += b.lo;
    if (FORM == MFORM_WIDE) a.hi += b.hi + (a.lo < b.lo ? 1ull : 0ull);
  }
}

// cells += t by atomics (LDS or HBM cells alike)
template <int FORM>
__device__ __forceinline__ void m_atomic(u64* s1, u64* lo, u64* hi, const MTerm& t) {
  if (FORM == MFORM_REAL) {
    atomicAdd(reinterpret_cast<double*>(s1), __longlong_as_double((long long)t.s1));
    atomicAdd(reinterpret_cast<double*>(lo), __longlong_as_double((long long)t.lo));
  } else if (FORM == MFORM_NARROW) {
    atomicAdd(s1, t.s1);
    atomicAdd(lo, t.lo);
  } else {
    atomicAdd(s1, t.s1);
    const u64 old = atomicAdd(lo, t.lo);
    const u64 up = t.hi + ((u64)(old + t.lo) < t.lo ? 1ull : 0ull);  // the term's high half and lo's carry
    if (up) atomicAdd(hi, up);
  }
}

template <int FORM>
__device__ __forceinline__ MTerm m_shuffle(const MTerm& t, int o) {
  MTerm r;
  r.s1 = (u64)__shfl_xor((long long)t.s1, o, 64);
  r.lo = (u64)__shfl_xor((long long)t.lo, o, 64);
  r.hi = FORM == MFORM_WIDE ? (u64)__shfl_xor((long long)t.hi, o, 64) : 0ull;
  return r;
}

constexpr int kMAggCells = 1 + 3 * kMMaxSlots;  // MODE_AGG: n and the slots' (S1, lo, hi) per wave in LDS

template <int MODE, int FORM>
__global__ void __launch_bounds__(kBlock) k_scan_moments(const MParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char m_lds[];
  u64* lds = reinterpret_cast<u64*>(m_lds);
  constexpr int CELLS = FORM == MFORM_WIDE ? 3 : 2;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ns = p.num_slots;
  const int64_t G = p.num_groups;
  const bool counting = p.n != nullptr;

  if (MODE == MODE_GROUP_LDS) {
    for (int64_t i = threadIdx.x; i < (int64_t)(1 + ns * CELLS) * G; i += kBlock) lds[i] = 0ull;  // (+0.0 too)
    __syncthreads();
  }

  u64 an = 0ull;
  MTerm acc[kMMaxSlots];
#pragma unroll
  for (int s = 0; s < kMMaxSlots; ++s) acc[s] = MTerm{0ull, 0ull, 0ull};

  for (int c = p.chunk_begin + (int)blockIdx.x; c < p.chunk_end; c += (int)gridDim.x) {
    const PH_CONST Chunk* ck = (const PH_CONST Chunk*)p.chunks + c;  // C-style cast = addrspacecast
    const int32_t seg = ck->seg, wb = ck->word_begin, we = ck->word_end;
    MSegPtr S = (MSegPtr)p.segs + seg;
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
          const MTerm t = m_term<FORM>(gld(S->d_of[v] + id));
          if (MODE == MODE_AGG) {
            m_combine<FORM>(acc[s], t);
          } else if (MODE == MODE_GROUP_LDS) {
            u64* base = lds + (int64_t)(1 + s * CELLS) * G + key;
            m_atomic<FORM>(base, base + G, base + 2 * G, t);  // (the hi cell is touched by MFORM_WIDE only)
          } else {
            m_atomic<FORM>(p.s1[s] + key, p.s2lo[s] + key, FORM == MFORM_WIDE ? p.s2hi[s] + key : nullptr, t);
          }
        }
      }
    }
    if (counting && lane == 0 && pc) atomicAdd(p.seg_count + seg, pc);
  }

  if (MODE == MODE_AGG) {
    // wave reductions by shuffles (the wide form moves both halves and carries), the workgroup's waves combined in
    // LDS, one set of atomics per workgroup per slot
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) an += (u64)__shfl_xor((long long)an, o, 64);
    if (lane == 0) lds[wave * kMAggCells] = an;
#pragma unroll
    for (int s = 0; s < kMMaxSlots; ++s) {
      if (s < ns) {
        MTerm v = acc[s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m_combine<FORM>(v, m_shuffle<FORM>(v, o));
        if (lane == 0) {
          u64* cell = lds + wave * kMAggCells + 1 + 3 * s;
          cell[0] = v.s1;
          cell[1] = v.lo;
          cell[2] = v.hi;
        }
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < ns) {
      const int s = (int)threadIdx.x;
      MTerm v{0ull, 0ull, 0ull};
      u64 docs = 0ull;
      for (int k = 0; k < kWaves; ++k) {
        const u64* cell = lds + k * kMAggCells + 1 + 3 * s;
        m_combine<FORM>(v, MTerm{cell[0], cell[1], cell[2]});
        docs += lds[k * kMAggCells];
      }
      if (docs) {
        m_atomic<FORM>(p.s1[s], p.s2lo[s], FORM == MFORM_WIDE ? p.s2hi[s] : nullptr, v);
        if (s == 0 && counting) atomicAdd(p.n, docs);
      }
    }
  } else if (MODE == MODE_GROUP_LDS) {
    __syncthreads();
    for (int64_t g = threadIdx.x; g < G; g += kBlock) {
      const u64 docs = lds[g];  // (0 everywhere in a launch that does not count)
      if (docs) atomicAdd(p.n + g, docs);
#pragma unroll
      for (int s = 0; s < kMMaxSlots; ++s) {
        if (s < ns) {
          const u64* base = lds + (int64_t)(1 + s * CELLS) * G + g;
          const MTerm v{base[0], base[G], FORM == MFORM_WIDE ? base[2 * G] : 0ull};
          if (v.s1 | v.lo | v.hi)  // (all zero adds nothing: a group the workgroup saw no doc of, mostly)
            m_atomic<FORM>(p.s1[s] + g, p.s2lo[s] + g, FORM == MFORM_WIDE ? p.s2hi[s] + g : nullptr, v);
        }
      }
    }
  }
}

// ---- finish: (n, S1, S2) -> VarianceTuple

__global__ void __launch_bounds__(256) k_moments_finish(const MFinishParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.num_groups * p.num_slots) return;
  const int s = (int)(i / p.num_groups);
  const int64_t g = i - (int64_t)s * p.num_groups;
  const u64 n = gld(p.n + g);
  MTuple out{(int64_t)n, 0.0, 0.0};
  if (n) {
    const u64 s1 = gld(p.s1[s] + g), lo = gld(p.s2lo[s] + g);
    if (p.form[s] == MFORM_REAL) {
      const double k = __longlong_as_double(p.shift[s]), a = __longlong_as_double((long long)s1);
      const double dn = (double)n;
      out.sum = dn * k + a;
      out.m2 = fmax(0.0, __longlong_as_double((long long)lo) - a * a / dn);
    } else {
      const u64 hi = p.form[s] == MFORM_WIDE ? gld(p.s2hi[s] + g) : 0ull;
      // sum = n K + S1 as a 128-bit two's complement integer, then its magnitude rounded once
      const long long K = p.shift[s];
      const u64 ka = K < 0 ? 0ull - (u64)K : (u64)K;
      u64 tl = n * ka, th = __umul64hi(n, ka);
      if (K < 0) {
        tl = ~tl + 1ull;
        th = ~th + (tl == 0ull ? 1ull : 0ull);
      }
      const u64 ext = (long long)s1 < 0 ? ~0ull : 0ull;
      const u64 sl = tl + s1;
      u64 sh = th + ext + (sl < tl ? 1ull : 0ull);
      const bool neg = (long long)sh < 0;
      u64 ml = sl;
      if (neg) {
        ml = ~sl + 1ull;
        sh = ~sh + (ml == 0ull ? 1ull : 0ull);
      }
      const u64 sum_limbs[4] = {ml, sh, 0ull, 0ull};
      const double mag = m_limbs_to_double(sum_limbs);
      out.sum = neg ? -mag : mag;
      // m2 = (n S2 - S1^2) / n: the numerator exactly in four limbs (>= 0 by Cauchy-Schwarz), rounded once, and one
      // division by (double) n (exact: n < 2^53)
      u64 x[4];
      x[0] = n * lo;
      const u64 c0 = __umul64hi(n, lo), p1 = n * hi, c1 = __umul64hi(n, hi);
      x[1] = c0 + p1;
      x[2] = c1 + (x[1] < c0 ? 1ull : 0ull);
      x[3] = 0ull;
      const u64 a = (long long)s1 < 0 ? 0ull - s1 : s1;
      const u64 q[4] = {a * a, __umul64hi(a, a), 0ull, 0ull};
      u64 borrow = 0ull;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const u64 d1 = x[k] - q[k];
        const u64 b1 = x[k] < q[k] ? 1ull : 0ull;
        const u64 d2 = d1 - borrow;
        const u64 b2 = d1 < borrow ? 1ull : 0ull;
        x[k] = d2;
        borrow = b1 | b2;
      }
      out.m2 = m_limbs_to_double(x) / (double)n;
    }
  }
  p.out[s][g] = out;
}

size_t moments_lds_bytes(const MParams& p, int mode, int form) {
  if (mode == MODE_AGG) return (size_t)kWaves * kMAggCells * 8;
  if (mode == MODE_GROUP_LDS) return (size_t)(1 + p.num_slots * (form == MFORM_WIDE ? 3 : 2)) * (size_t)p.num_groups * 8;
  return 0;
}

template <int MODE>
static void launch_mode(const MParams& p, int form, int grid, size_t lds, hipStream_t s) {
  switch (form) {
    case MFORM_NARROW:
      allow_lds(k_scan_moments<MODE, MFORM_NARROW>, lds);
      hipLaunchKernelGGL((k_scan_moments<MODE, MFORM_NARROW>), dim3(grid), dim3(kBlock), lds, s, p);
      break;
    case MFORM_WIDE:
      allow_lds(k_scan_moments<MODE, MFORM_WIDE>, lds);
      hipLaunchKernelGGL((k_scan_moments<MODE, MFORM_WIDE>), dim3(grid), dim3(kBlock), lds, s, p);
      break;
    case MFORM_REAL:
      allow_lds(k_scan_moments<MODE, MFORM_REAL>, lds);
      hipLaunchKernelGGL((k_scan_moments<MODE, MFORM_REAL>), dim3(grid), dim3(kBlock), lds, s, p);
      break;
    default: fail(PH_ERR_INVALID_ARGUMENT, "moments scan with a bad form");
  }
}

void launch_scan_moments(const MParams& p, int mode, int form, int grid, hipStream_t s) {
  if (!p.segs || !p.chunks || p.num_slots <= 0 || p.num_slots > kMMaxSlots || p.num_group_cols < 0 ||
      p.num_group_cols > kMaxGroupCols || p.num_groups <= 0 || (p.n == nullptr) != (p.seg_count == nullptr) ||
      grid <= 0)
    fail(PH_ERR_INVALID_ARGUMENT, "moments scan with bad parameters");
  for (int i = 0; i < p.num_slots; ++i)
    if (!p.s1[i] || !p.s2lo[i] || (form == MFORM_WIDE && !p.s2hi[i]) || p.slot_col[i] < 0 || p.slot_col[i] >= kMMaxSlots)
      fail(PH_ERR_INVALID_ARGUMENT, "moments scan with a bad slot");
  const size_t lds = moments_lds_bytes(p, mode, form);
  if (lds > 160 * 1024) fail(PH_ERR_INVALID_ARGUMENT, "moments scan tables exceed the LDS of one CU");
  switch (mode) {
    case MODE_AGG: launch_mode<MODE_AGG>(p, form, grid, lds, s); break;
    case MODE_GROUP_LDS: launch_mode<MODE_GROUP_LDS>(p, form, grid, lds, s); break;
    case MODE_GROUP_GLOBAL: launch_mode<MODE_GROUP_GLOBAL>(p, form, grid, lds, s); break;
    default: fail(PH_ERR_UNSUPPORTED, "variance moments in this plan mode");
  }
  PH_HIP_CHECK(hipGetLastError());
}

void launch_moments_finish(const MFinishParams& p, hipStream_t s) {
  if (p.num_groups <= 0 || p.num_slots <= 0 || p.num_slots > kMMaxSlots || !p.n)
    fail(PH_ERR_INVALID_ARGUMENT, "moments finish with bad parameters");
  const int64_t threads = p.num_groups * p.num_slots;
  hipLaunchKernelGGL(k_moments_finish, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, p);
  PH_HIP_CHECK(hipGetLastError());
}

}  // namespace ph
