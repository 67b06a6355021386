// scan_comoments.hip -- COVAR_POP / COVAR_SAMP as exact shifted co-moments.
//
// The reference adds sumX += x, sumY += y, sumXY += x y, count += 1 per doc in doubles (CovarianceAggregationFunction.
// java:95-140, CovarianceTuple.apply).  Here the planner (comoments.cpp) takes Kx, Ky, the smallest value of each
// argument column over the call's segments, so dx = x - Kx and dy = y - Ky are unsigned and every product is
// non-negative; the scan accumulates n, S1x = sum(dx), S1y = sum(dy) and Sxy = sum(dx dy) per group, exact integers in
// the integer forms, and k_comoments_finish turns them into the reference's tuple, every component rounded once.
//
// Decode is reg_decode.h's: a wave takes 2048-doc tiles of a chunk, lane l owns the 32 consecutive docs
// [32 l, 32 l + 32) and holds each stream's b-bit dictIds as b dwords.  The lane's 32 mask bits are half l % 2 of word
// l / 2 of the WHERE clause's bitmap (all ones without one, the bits past num_docs cleared); a tile whose masks are
// zero across the wave issues no stream load.  Per tile the first group-by stream, x and y are unpacked one after the
// other, the next tile's loads are issued (its mask was fetched at the top of this tile), and only then the lane walks
// its docs: the d_of gathers (dictionary-sized tables, L2-resident) and the accumulation run under the next tile's
// loads.  A launch's slots are scanned one after the other (the pool holds one tile of three streams, whatever the
// number of slots); further group-by columns are loaded inside the tile, without a prefetch.
//   MODE_AGG           per-lane (n, S1x, S1y, Sxy) over the whole chunk loop, a wave reduction by shuffles, the four
//                      waves combined in LDS, one set of atomics per workgroup per slot
//   MODE_GROUP_LDS     a lane keeps a running (key, n, S1x, S1y, Sxy) over its 32 docs and issues atomics only when the
//                      key changes or the run ends: into per-workgroup LDS tables -- n[G], then per slot S1x[G], S1y[G],
//                      Sxy[G] and (wide) Sxy hi[G] -- flushed to the HBM tables at the end (all-zero cells are skipped)
//   MODE_GROUP_GLOBAL  the same adds, straight into the HBM tables
//   CFORM_NARROW       Sxy is one u64 (the planner's bound: it never carries): no-return atomics only
//   CFORM_WIDE         dx dy is a 64 x 64 -> 128 product added into a (lo, hi) pair with an explicit carry; in a table
//                      the add of the low half returns the old value, and the carry it shows goes into the high half
//   CFORM_REAL         x, y and the three sums are doubles (no shift), atomicAdd on doubles
// The docs matched per segment (popcounts of the masks, one atomic per wave and run of tiles of one segment) give the
// statistics.
#include <algorithm>

#include "limbs_to_double.h"
#include "reg_decode.h"

namespace ph {

typedef const PH_CONST CSegment* CSegPtr;
typedef unsigned long long u64;

// what one doc, or one run of docs, adds to a slot: S1x, S1y and Sxy as (lo, hi); doubles' bits in CFORM_REAL
struct CTerm {
  u64 sx, sy, lo, hi;
};

__device__ __forceinline__ double c_f64(u64 b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ u64 c_bits(double x) { return (u64)__double_as_longlong(x); }

// a += the doc (x, y), the table entries of its two dictIds
template <int FORM>
__device__ __forceinline__ void c_add_doc(CTerm& a, u64 x, u64 y) {
  if (FORM == CFORM_REAL) {
    const double dx = c_f64(x), dy = c_f64(y);
    a.sx = c_bits(c_f64(a.sx) + dx);
    a.sy = c_bits(c_f64(a.sy) + dy);
    a.lo = c_bits(c_f64(a.lo) + dx * dy);
  } else {
    a.sx += x;
    a.sy += y;
    const u64 lo = x * y;  // all of the product in CFORM_NARROW (the planner's bound)
    a.lo += lo;
    if (FORM == CFORM_WIDE) a.hi += __umul64hi(x, y) + (a.lo < lo ? 1ull : 0ull);
  }
}

// a += b in registers
template <int FORM>
__device__ __forceinline__ void c_combine(CTerm& a, const CTerm& b) {
  if (FORM == CFORM_REAL) {
    a.sx = c_bits(c_f64(a.sx) + c_f64(b.sx));
    a.sy = c_bits(c_f64(a.sy) + c_f64(b.sy));
    a.lo = c_bits(c_f64(a.lo) + c_f64(b.lo));
  } else {
    a.sx += b.sx;
    a.sy += b.sy;
    a.lo += b.lo;
    if (FORM == CFORM_WIDE) a.hi += b.hi + (a.lo < b.lo ? 1ull : 0ull);
  }
}

// cells += t by atomics (LDS or HBM cells alike)
template <int FORM>
__device__ __forceinline__ void c_atomic(u64* sx, u64* sy, u64* lo, u64* hi, const CTerm& t) {
  if (FORM == CFORM_REAL) {
    atomicAdd(reinterpret_cast<double*>(sx), c_f64(t.sx));
    atomicAdd(reinterpret_cast<double*>(sy), c_f64(t.sy));
    atomicAdd(reinterpret_cast<double*>(lo), c_f64(t.lo));
  } else {
    atomicAdd(sx, t.sx);
    atomicAdd(sy, t.sy);
    if (FORM == CFORM_NARROW) {
      atomicAdd(lo, t.lo);
    } else {
      const u64 old = atomicAdd(lo, t.lo);
      const u64 up = t.hi + ((u64)(old + t.lo) < t.lo ? 1ull : 0ull);  // the term's high half and lo's carry
      if (up) atomicAdd(hi, up);
    }
  }
}

template <int FORM>
__device__ __forceinline__ CTerm c_shuffle(const CTerm& t, int o) {
  CTerm r;
  r.sx = (u64)__shfl_xor((long long)t.sx, o, 64);
  r.sy = (u64)__shfl_xor((long long)t.sy, o, 64);
  r.lo = (u64)__shfl_xor((long long)t.lo, o, 64);
  r.hi = FORM == CFORM_WIDE ? (u64)__shfl_xor((long long)t.hi, o, 64) : 0ull;
  return r;
}

constexpr int kCAggCells = 5;  // MODE_AGG: (n, S1x, S1y, lo, hi) per wave and slot in LDS

template <int MODE, int FORM, int C>
__global__ void __launch_bounds__(kBlock) k_scan_comoments(const CParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char c_lds[];
  u64* lds = reinterpret_cast<u64*>(c_lds);
  constexpr int CELLS = FORM == CFORM_WIDE ? 4 : 3;
  constexpr int32_t TW = kRegTileWords;
  constexpr int32_t round_words = kWaves * TW;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ns = p.num_slots;
  const int ng = p.num_group_cols;
  const uint32_t G = (uint32_t)p.num_groups;
  CSegPtr segs = (CSegPtr)p.segs;
  const PH_CONST Chunk* chunks = (const PH_CONST Chunk*)p.chunks;  // C-style cast = addrspacecast
  const PH_CONST CSlot* slots = (const PH_CONST CSlot*)p.slots;

  if (MODE == MODE_GROUP_LDS) {
    for (int64_t i = threadIdx.x; i < (int64_t)(1 + ns * CELLS) * G; i += kBlock) lds[i] = 0ull;  // (+0.0 too)
    __syncthreads();
  }

  const int64_t nch = p.chunk_end - p.chunk_begin;
  const int32_t c_begin = p.chunk_begin + (int32_t)(nch * blockIdx.x / gridDim.x);
  const int32_t c_end = p.chunk_begin + (int32_t)(nch * (blockIdx.x + 1) / gridDim.x);
  struct Tile {
    CSegPtr S;
    int32_t seg, w0, ndoc;
  };
  struct Pool {
    u32x4 g[C], x[C], y[C];
  };
  auto stream_bytes = [](int32_t docs, int32_t bits) { return ((int64_t)docs * bits + 7) / 8; };

#pragma unroll 1
  for (int s = 0; s < ns; ++s) {  // wave-uniform
    const int v = slots[s].pair;
    const bool counting = s == 0 && p.n != nullptr;
    int32_t c = c_begin, r = 0;
    auto next_tile = [&]() {
      Tile t{nullptr, 0, 0, 0};
      if (c < c_end) {
        const int32_t cbeg = chunks[c].word_begin, cend = chunks[c].word_end;
        t.seg = chunks[c].seg;
        t.S = segs + t.seg;
        t.w0 = cbeg + r * round_words + wave * TW;
        const int32_t nw = min(TW, cend - t.w0);
        t.ndoc = nw > 0 ? max(0, min(nw * 64, t.S->num_docs - t.w0 * 64)) : 0;
        if (cbeg + (r + 1) * round_words < cend) {
          ++r;
        } else {
          ++c;
          r = 0;
        }
      }
      return t;
    };
    // the lane's 32 mask bits of a tile: docs [32 lane, 32 lane + 32) of it, word w0 + lane / 2 of the bitmap
    auto mask_of = [&](const Tile& t) -> uint32_t {
      const int32_t nv = max(0, min(32, t.ndoc - lane * 32));
      uint32_t m = nv >= 32 ? 0xffffffffu : ((1u << nv) - 1u);
      const u64* bm = t.ndoc > 0 ? t.S->mask : nullptr;  // (wave-uniform)
      if (bm && nv > 0) m &= (uint32_t)(gld(bm + t.w0 + (lane >> 1)) >> ((lane & 1) * 32));
      return m;
    };
    auto load = [&](const Tile& t, bool use, Pool& pl) {
      use = use && t.ndoc > 0;
      const bool live = use && lane * 32 < t.ndoc;
      const int32_t nd = use ? t.S->num_docs : 0;
      const bool grp = use && MODE != MODE_AGG && ng > 0;
      const int32_t gb = grp ? t.S->gbits[0] : 0, xb = use ? t.S->pair[v].xbits : 0, yb = use ? t.S->pair[v].ybits : 0;
      if (MODE != MODE_AGG)
        reg_load<C>(grp, live, grp ? t.S->gfwd[0] : nullptr, gb, stream_bytes(nd, gb), t.w0 * 2, lane, pl.g);
      reg_load<C>(use, live, use ? t.S->pair[v].xfwd : nullptr, xb, stream_bytes(nd, xb), t.w0 * 2, lane, pl.x);
      reg_load<C>(use, live, use ? t.S->pair[v].yfwd : nullptr, yb, stream_bytes(nd, yb), t.w0 * 2, lane, pl.y);
    };

    u64* const t_sx = slots[s].s1x;
    u64* const t_sy = slots[s].s1y;
    u64* const t_lo = slots[s].sxy;
    u64* const t_hi = slots[s].sxyhi;
    u64* const l_sx = lds + (int64_t)(1 + s * CELLS) * G;  // MODE_GROUP_LDS: this slot's cells
    // the run [key, n, terms) of a lane ends: one set of atomics
    auto flush = [&](uint32_t key, u64 docs, const CTerm& run) {
      if (key >= G) return;  // (never: remapped ids index the call's dictionaries)
      if (MODE == MODE_GROUP_LDS) {
        if (counting) atomicAdd(lds + key, docs);
        c_atomic<FORM>(l_sx + key, l_sx + G + key, l_sx + 2 * (int64_t)G + key, l_sx + 3 * (int64_t)G + key, run);
      } else {
        if (counting) atomicAdd(p.n + key, docs);
        c_atomic<FORM>(t_sx + key, t_sy + key, t_lo + key, FORM == CFORM_WIDE ? t_hi + key : nullptr, run);
      }
    };

    u64 an = 0ull;   // per lane: matched docs of the slot's scan
    u64 pc = 0ull;   // per lane: matched docs of the tiles of segment `pc_seg` so far
    int32_t pc_seg = -1;
    CTerm acc{0ull, 0ull, 0ull, 0ull};
    auto count_flush = [&]() {
      const u64 docs = (u64)wave_sum_i64((int64_t)pc);
      if (lane == 0 && docs) atomicAdd(p.seg_count + pc_seg, docs);
      pc = 0ull;
    };

    Pool pl;
    Tile t = next_tile();
    uint32_t m = mask_of(t);
    bool any = __ballot(m != 0u) != 0ull;
    load(t, any, pl);
    while (t.S != nullptr) {  // wave-uniform
      const Tile tn = next_tile();
      const uint32_t mn = mask_of(tn);  // (its load runs under this tile's unpacks)
      if (counting && t.seg != pc_seg) {
        if (pc_seg >= 0) count_flush();
        pc_seg = t.seg;
      }
      pc += (u64)__builtin_popcount(m);
      an += (u64)__builtin_popcount(m);
      uint32_t key[MODE == MODE_AGG ? 1 : 32], xid[32], yid[32];
      const unsigned long long* x_of = nullptr;
      const unsigned long long* y_of = nullptr;
      if (any) {
        CSegPtr S = t.S;
        if constexpr (MODE != MODE_AGG) {
          if (ng > 0) {
            reg_unpack<C>(pl.g, S->gbits[0], key);
            const int32_t* rm = S->gremap[0];
            const uint32_t st = p.group_stride[0];
#pragma unroll
            for (int j = 0; j < 32; ++j) {
              uint32_t id = ((m >> j) & 1u) ? key[j] : 0u;
              if (rm) id = (uint32_t)gld(rm + id);
              key[j] = id * st;
            }
          } else {
#pragma unroll
            for (int j = 0; j < 32; ++j) key[j] = 0u;
          }
#pragma unroll
          for (int g = 1; g < kMaxGroupCols; ++g) {
            if (g < ng) {  // further group-by columns: loaded here, into the first one's registers
              const int32_t gb = S->gbits[g];
              reg_load<C>(true, lane * 32 < t.ndoc, S->gfwd[g], gb, stream_bytes(S->num_docs, gb), t.w0 * 2, lane, pl.g);
              reg_unpack<C>(pl.g, gb, xid);
              const int32_t* rm = S->gremap[g];
              const uint32_t st = p.group_stride[g];
#pragma unroll
              for (int j = 0; j < 32; ++j) {
                uint32_t id = ((m >> j) & 1u) ? xid[j] : 0u;
                if (rm) id = (uint32_t)gld(rm + id);
                key[j] += id * st;
              }
            }
          }
        }
        reg_unpack<C>(pl.x, S->pair[v].xbits, xid);
        reg_unpack<C>(pl.y, S->pair[v].ybits, yid);
        x_of = S->pair[v].x_of;
        y_of = S->pair[v].y_of;
      }
      const bool anyn = __ballot(mn != 0u) != 0ull;
      load(tn, anyn, pl);
      if (any) {
        // an unmatched doc reads entry 0 of the tables (always there) and adds nothing: no branch per doc
        if constexpr (MODE == MODE_AGG) {
#pragma unroll
          for (int j = 0; j < 32; ++j) {
            const bool hit = (m >> j) & 1u;
            const u64 x = gld(x_of + (hit ? xid[j] : 0u)), y = gld(y_of + (hit ? yid[j] : 0u));
            c_add_doc<FORM>(acc, hit ? x : 0ull, hit ? y : 0ull);
          }
        } else {
          uint32_t ck = 0u;
          u64 docs = 0ull;
          CTerm run{0ull, 0ull, 0ull, 0ull};
#pragma unroll
          for (int j = 0; j < 32; ++j) {
            const bool hit = (m >> j) & 1u;
            const u64 x = gld(x_of + (hit ? xid[j] : 0u)), y = gld(y_of + (hit ? yid[j] : 0u));
            const uint32_t kj = hit ? key[j] : ck;  // (an unmatched doc never ends a run)
            if (kj != ck) {
              if (docs) flush(ck, docs, run);
              docs = 0ull;
              run = CTerm{0ull, 0ull, 0ull, 0ull};
              ck = kj;
            }
            docs += hit ? 1ull : 0ull;
            c_add_doc<FORM>(run, hit ? x : 0ull, hit ? y : 0ull);
          }
          if (docs) flush(ck, docs, run);
        }
      }
      t = tn;
      m = mn;
      any = anyn;
    }
    if (counting && pc_seg >= 0) count_flush();

    if (MODE == MODE_AGG) {
      // wave reductions by shuffles (the wide form moves both halves and carries); lane 0 parks the wave's sums in LDS
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) an += (u64)__shfl_xor((long long)an, o, 64);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c_combine<FORM>(acc, c_shuffle<FORM>(acc, o));
      if (lane == 0) {
        u64* cell = lds + (wave * kCMaxSlots + s) * kCAggCells;
        cell[0] = an;
        cell[1] = acc.sx;
        cell[2] = acc.sy;
        cell[3] = acc.lo;
        cell[4] = acc.hi;
      }
    }
  }

  if (MODE == MODE_AGG) {
    // the workgroup's waves combined, one set of atomics per workgroup per slot
    __syncthreads();
    if ((int)threadIdx.x < ns) {
      const int s = (int)threadIdx.x;
      CTerm t{0ull, 0ull, 0ull, 0ull};
      u64 docs = 0ull;
      for (int k = 0; k < kWaves; ++k) {
        const u64* cell = lds + (k * kCMaxSlots + s) * kCAggCells;
        docs += cell[0];
        c_combine<FORM>(t, CTerm{cell[1], cell[2], cell[3], cell[4]});
      }
      if (docs) {
        c_atomic<FORM>(slots[s].s1x, slots[s].s1y, slots[s].sxy, FORM == CFORM_WIDE ? slots[s].sxyhi : nullptr, t);
        if (s == 0 && p.n != nullptr) atomicAdd(p.n, docs);
      }
    }
  } else if (MODE == MODE_GROUP_LDS) {
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < G; g += kBlock) {
      const u64 docs = lds[g];  // (0 everywhere in a launch that does not count)
      if (docs) atomicAdd(p.n + g, docs);
      for (int s = 0; s < ns; ++s) {
        const u64* base = lds + (int64_t)(1 + s * CELLS) * G + g;
        const CTerm t{base[0], base[G], base[2 * (int64_t)G], FORM == CFORM_WIDE ? base[3 * (int64_t)G] : 0ull};
        if (t.sx | t.sy | t.lo | t.hi)  // (all zero adds nothing: a group the workgroup saw no doc of, mostly)
          c_atomic<FORM>(slots[s].s1x + g, slots[s].s1y + g, slots[s].sxy + g,
                         FORM == CFORM_WIDE ? slots[s].sxyhi + g : nullptr, t);
      }
    }
  }
}

// ---- finish: (n, S1x, S1y, Sxy) -> CovarianceTuple

// a 256-bit two's complement integer (four limbs, a[0] lowest) += or -= x y z, three unsigned 64-bit factors whose
// product stays below 2^192
__device__ __forceinline__ void c_addmul(u64 (&a)[4], bool neg, u64 x, u64 y, u64 z) {
  const u64 p0 = x * y, p1 = __umul64hi(x, y);
  u64 q[4];
  q[0] = p0 * z;
  const u64 c0 = __umul64hi(p0, z), t0 = p1 * z, t1 = __umul64hi(p1, z);
  q[1] = c0 + t0;
  q[2] = t1 + (q[1] < c0 ? 1ull : 0ull);
  q[3] = 0ull;
  u64 carry = 0ull;  // (or the borrow)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (neg) {
      const u64 d1 = a[k] - q[k], b1 = a[k] < q[k] ? 1ull : 0ull;
      const u64 d2 = d1 - carry, b2 = d1 < carry ? 1ull : 0ull;
      a[k] = d2;
      carry = b1 | b2;
    } else {
      const u64 s1 = a[k] + q[k], c1 = s1 < q[k] ? 1ull : 0ull;
      const u64 s2 = s1 + carry, c2 = s2 < carry ? 1ull : 0ull;
      a[k] = s2;
      carry = c1 | c2;
    }
  }
}

// the 256-bit two's complement integer as a double: its magnitude rounded once to nearest-even
__device__ __forceinline__ double c_signed_to_double(const u64 (&a)[4]) {
  const bool neg = (a[3] >> 63) != 0ull;
  u64 mag[4];
  u64 carry = 1ull;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (neg) {
      mag[k] = ~a[k] + carry;
      carry = (carry && mag[k] == 0ull) ? 1ull : 0ull;
    } else {
      mag[k] = a[k];
    }
  }
  const double d = m_limbs_to_double(mag);
  return neg ? -d : d;
}

__device__ __forceinline__ u64 c_abs(long long k) { return k < 0 ? 0ull - (u64)k : (u64)k; }

__global__ void __launch_bounds__(256) k_comoments_finish(const CFinishParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.num_groups * p.num_slots) return;
  const int sl = (int)(i / p.num_groups);
  const int64_t g = i - (int64_t)sl * p.num_groups;
  // (static indices into the by-value parameter arrays: a dynamic one would copy them to scratch)
  int form = 0;
  long long kx = 0, ky = 0;
  const u64 *ps1x = nullptr, *ps1y = nullptr, *psxy = nullptr, *phi = nullptr;
  CTuple* dst = nullptr;
#pragma unroll
  for (int k = 0; k < kCMaxSlots; ++k)
    if (k == sl) {
      form = p.form[k];
      kx = p.kx[k];
      ky = p.ky[k];
      ps1x = p.s1x[k];
      ps1y = p.s1y[k];
      psxy = p.sxy[k];
      phi = p.sxyhi[k];
      dst = p.out[k];
    }
  const u64 n = gld(p.n + g);
  // no doc: the reference's empty holder, CovarianceTuple(0.0, 0.0, 0.0, 0) (CovarianceAggregationFunction.java:155-162)
  CTuple out{0.0, 0.0, 0.0, (int64_t)n};
  if (n) {
    const u64 s1x = gld(ps1x + g), s1y = gld(ps1y + g), lo = gld(psxy + g);
    if (form == CFORM_REAL) {
      out.sum_x = c_f64(s1x);
      out.sum_y = c_f64(s1y);
      out.sum_xy = c_f64(lo);
    } else {
      const u64 hi = form == CFORM_WIDE ? gld(phi + g) : 0ull;
      // sum(x) = n Kx + S1x, sum(y) likewise, sum(x y) = Sxy + Ky S1x + Kx S1y + n Kx Ky: exact, then rounded once
      u64 a[4] = {s1x, 0ull, 0ull, 0ull};
      c_addmul(a, kx < 0, n, c_abs(kx), 1ull);
      out.sum_x = c_signed_to_double(a);
      u64 b[4] = {s1y, 0ull, 0ull, 0ull};
      c_addmul(b, ky < 0, n, c_abs(ky), 1ull);
      out.sum_y = c_signed_to_double(b);
      u64 c[4] = {lo, hi, 0ull, 0ull};
      c_addmul(c, ky < 0, s1x, c_abs(ky), 1ull);
      c_addmul(c, kx < 0, s1y, c_abs(kx), 1ull);
      c_addmul(c, (kx < 0) != (ky < 0), c_abs(kx), c_abs(ky), n);
      out.sum_xy = c_signed_to_double(c);
    }
  }
  dst[g] = out;
}

size_t comoments_lds_bytes(const CParams& p, int mode, int form) {
  if (mode == MODE_AGG) return (size_t)kWaves * kCMaxSlots * kCAggCells * 8;
  if (mode == MODE_GROUP_LDS) return (size_t)(1 + p.num_slots * (form == CFORM_WIDE ? 4 : 3)) * (size_t)p.num_groups * 8;
  return 0;
}

template <int MODE, int FORM>
static void launch_form(const CParams& p, int max_bits, int grid, size_t lds, hipStream_t s) {
  // a lane's dwords of a b-bit stream sit in b / 4 (rounded up) 16-byte registers: 4 of them to 16 bits, 8 to 32
  if (max_bits <= 16) {
    allow_lds(k_scan_comoments<MODE, FORM, 4>, lds);
    hipLaunchKernelGGL((k_scan_comoments<MODE, FORM, 4>), dim3(grid), dim3(kBlock), lds, s, p);
  } else {
    allow_lds(k_scan_comoments<MODE, FORM, 8>, lds);
    hipLaunchKernelGGL((k_scan_comoments<MODE, FORM, 8>), dim3(grid), dim3(kBlock), lds, s, p);
  }
}

template <int MODE>
static void launch_mode(const CParams& p, int form, int max_bits, int grid, size_t lds, hipStream_t s) {
  switch (form) {
    case CFORM_NARROW: launch_form<MODE, CFORM_NARROW>(p, max_bits, grid, lds, s); break;
    case CFORM_WIDE: launch_form<MODE, CFORM_WIDE>(p, max_bits, grid, lds, s); break;
    case CFORM_REAL: launch_form<MODE, CFORM_REAL>(p, max_bits, grid, lds, s); break;
    default: fail(PH_ERR_INVALID_ARGUMENT, "co-moments scan with a bad form");
  }
}

void launch_scan_comoments(const CParams& p, int mode, int form, int max_bits, int grid, hipStream_t s) {
  if (!p.segs || !p.chunks || !p.slots || p.num_slots <= 0 || p.num_slots > kCMaxSlots || p.num_group_cols < 0 ||
      p.num_group_cols > kMaxGroupCols || p.num_groups <= 0 || p.num_groups > 0xffffffffll ||
      (p.n == nullptr) != (p.seg_count == nullptr) || max_bits < 1 || max_bits > 32 || grid <= 0)
    fail(PH_ERR_INVALID_ARGUMENT, "co-moments scan with bad parameters");
  const size_t lds = comoments_lds_bytes(p, mode, form);
  if (lds > 160 * 1024) fail(PH_ERR_INVALID_ARGUMENT, "co-moments scan tables exceed the LDS of one CU");
  switch (mode) {
    case MODE_AGG: launch_mode<MODE_AGG>(p, form, max_bits, grid, lds, s); break;
    case MODE_GROUP_LDS: launch_mode<MODE_GROUP_LDS>(p, form, max_bits, grid, lds, s); break;
    case MODE_GROUP_GLOBAL: launch_mode<MODE_GROUP_GLOBAL>(p, form, max_bits, grid, lds, s); break;
    default: fail(PH_ERR_UNSUPPORTED, "co-moments in this plan mode");
  }
  PH_HIP_CHECK(hipGetLastError());
}

void launch_comoments_finish(const CFinishParams& p, hipStream_t s) {
  if (p.num_groups <= 0 || p.num_slots <= 0 || p.num_slots > kCMaxSlots || !p.n)
    fail(PH_ERR_INVALID_ARGUMENT, "co-moments finish with bad parameters");
  const int64_t threads = p.num_groups * p.num_slots;
  hipLaunchKernelGGL(k_comoments_finish, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, p);
  PH_HIP_CHECK(hipGetLastError());
}

}  // namespace ph
