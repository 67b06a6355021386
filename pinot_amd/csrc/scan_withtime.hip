// scan_withtime.hip -- FIRSTWITHTIME / LASTWITHTIME(dataCol, timeCol, 'type'): per result row, the value of the doc
// with the extreme time.
//
// The reference walks a block's docs in ascending docId and replaces its (value, time) pair on `time >= lastTime`
// (LastWithTimeAggregationFunction.java:123-128, 172-177; LastIntValueWithTimeAggregationFunction.java:65-93) or
// `time <= firstTime` (FirstWithTimeAggregationFunction.java:122-127, 171-176), the time being timeValSet.
// getLongValuesSV().  So in both directions the doc with the largest docId wins among those with the extreme time;
// merge keeps its first argument on equal times (:200-206), which this plan applies in the call's segment order.
//
// Cell.  A slot is one (time column, direction) pair; every aggregation over it selects the same doc, whatever its
// data column, so a row holds one uint64 per slot:
//   K = hi_of[dictId(time)] << 32 | (0xFFFFFFFF - ord),   ord = base[segment] + (docs of the segment - 1 - doc).
// hi_of comes from the planner (withtime.cpp): rank + 1 of the doc's (long) time among the call's distinct times for
// LAST, T - rank for FIRST, so the scan always maximises and 0 is the empty cell.  A larger K is a better time, then an
// earlier segment, then a larger docId.  The data columns are not read here: k_withtime_finish gathers one value per
// result cell from the doc the cell names.
//
// hi_of tables.  When the tables of every slot fit WParams::tab_bytes (the planner's budget, the context option
// withtime_table_lds_max) a workgroup stages the current segment's tables into LDS, as k_scan_bins stages its bin
// tables; otherwise the lookup is a gather from HBM.
//
//   MODE_AGG           every lane keeps a running maximum per slot in registers over all its docs: no atomics and no LDS
//                      traffic in the loop.  At the end a wave maximum by shuffles, one LDS cell per wave and slot, one
//                      HBM atomic max per workgroup and slot.
//                      REG = 1, register-direct (reg_decode.h), when every slot's packed time width is at most 16 bits:
//                      lane l owns docs [32 l, 32 l + 32) of a 2048-doc tile, whose keys ascend with the doc, so a tile
//                      is reduced with 32-bit compares of hi alone (`hi >= best` keeps the later doc) and joins the
//                      64-bit maximum once; a tile whose masks are zero across the wave issues no load.
//                      REG = 0, wider columns: lane l owns doc 64 w + l, decoded by unpack_bits.
//   MODE_GROUP_LDS     one zeroed workgroup table of G x slots cells (after n[G] when the query counts).
//     screen           per doc the cell is read with a plain LDS load and the doc dropped when K <= the value read.
//                      Cells only grow, so a stale read can only let a doc through, never drop a winner.  FIRST over
//                      ascending time drops nearly every doc here.
//     wave combine     the surviving lanes are combined before the atomic: the first lane still owing broadcasts its
//                      cell, a ballot finds the lanes with the same cell, the maximum of their keys (a wave reduction
//                      with the other lanes at 0) goes out as one LDS atomic max without return, and all of them retire.
//                      After WParams::combine_rounds rounds the lanes left issue their own atomics.  It is the match
//                      form of k_scan_bins with max in place of popcount, and matters for LAST over ascending time,
//                      where every doc passes the screen.
//                      The table is flushed at the end, non-zero cells only, with the same screen against HBM.
//   MODE_GROUP_GLOBAL  the same screen with a relaxed global load, the same combine, then an agent-scope atomic max.
// kWMatchRounds = 2 comes from counting instructions, not from a sweep: a round is ~12 scalar-side instructions for the
// match plus 6 shuffle steps of ~6 instructions for the 64-bit maximum, ~50 issue slots, while 64 lanes on distinct
// cells retire in one atomic instruction and m lanes on one cell serialise for ~m cycles.  A round therefore pays only
// when its row holds a large part of the wave; two rounds cover a wave split between two dominant rows (the boundary of
// two runs of a sorted group column) and stop there.  The one measurement taken ("With-time cells": 10M docs,
// 1 000 groups, MODE_GROUP_LDS) has the combine losing to one atomic per doc, 0.30 to 0.37 ms against 0.23 to 0.25 ms;
// MODE_GROUP_GLOBAL is unmeasured.  The context option withtime_no_combine runs with 0 rounds.
//
// n[G], for COUNT(*), is kept only when the query has one: equal rows of a wave are matched and the leader adds the
// popcount.  Without it a row exists exactly when slot 0's cell is not 0, which k_withtime_finish writes into n.
//
// k_withtime_finish: one thread per (row, with-time aggregation).  An empty cell gives the subclass's
// DEFAULT_VALUE_TIME_PAIR.  Otherwise ord comes from the cell's low word, the segment from a binary search over base[],
// the data column's dictId from unpack_bits at that doc, the value from the widened dictionary table (narrowed through
// float for FLOAT) and the time from time_of_rank, undoing FIRST's flip.
// All stores are plain vector stores; no inline assembly.
#include <algorithm>

#include "reg_decode.h"

namespace ph {

typedef const PH_CONST WSegment* WSegPtr;
typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// *cell = max(*cell, v) on an LDS or an HBM cell, result unused
__device__ __forceinline__ void w_max(u64* cell, u64 v, bool hbm) {
  if (hbm) (void)__hip_atomic_fetch_max(cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else (void)__hip_atomic_fetch_max(cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// the screen's read: whatever the cell held at some earlier moment
__device__ __forceinline__ u64 w_peek(const u64* cell, bool hbm) {
  if (hbm) return __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the cell index of the first lane of `owing` (not 0), on every lane
__device__ __forceinline__ int64_t w_leader_cell(int64_t cell, u64 owing) {
  const int leader = __ffsll((long long)owing) - 1;
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)cell, leader);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)((u64)cell >> 32), leader);
  return (int64_t)(((u64)hi << 32) | lo);
}

// the lanes of `mine` raise table[cell] to their key; lanes with equal cells are combined first.  Called by every lane
// of the wave: nothing here diverges, so the shuffles of the reduction see all 64 lanes
__device__ __forceinline__ void w_match_max(u64* table, int64_t cell, u64 key, bool mine, int lane, bool hbm, int rounds) {
#pragma unroll 1
  for (int round = 0; round < rounds; ++round) {
    const u64 owing = __ballot(mine);
    if (!owing) return;
    const int64_t lc = w_leader_cell(cell, owing);
    const bool same = mine && cell == lc;
    const u64 best = wave_max_u64(same ? key : 0ull);
    if (lane == __ffsll((long long)owing) - 1) w_max(table + lc, best, hbm);
    mine = mine && !same;
  }
  if (mine) w_max(table + cell, key, hbm);
}

// the same matching for n: the lanes of `mine` add 1 to table[cell]
__device__ __forceinline__ void w_match_count(u64* table, int64_t cell, bool mine, int lane, bool hbm, int rounds) {
#pragma unroll 1
  for (int round = 0; round < rounds; ++round) {
    const u64 owing = __ballot(mine);
    if (!owing) return;
    const int64_t lc = w_leader_cell(cell, owing);
    const bool same = mine && cell == lc;
    const u64 peers = __ballot(same);
    if (lane == __ffsll((long long)owing) - 1) {
      if (hbm) (void)__hip_atomic_fetch_add(table + lc, (u64)__popcll(peers), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else (void)__hip_atomic_fetch_add(table + lc, (u64)__popcll(peers), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    mine = mine && !same;
  }
  if (mine) {
    if (hbm) (void)__hip_atomic_fetch_add(table + cell, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else (void)__hip_atomic_fetch_add(table + cell, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

template <int MODE, int REG>
__global__ void __launch_bounds__(kBlock) k_scan_withtime(const WParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char w_lds[];
  uint32_t* lds_tab = reinterpret_cast<uint32_t*>(w_lds);
  u64* lds_n = reinterpret_cast<u64*>(w_lds + p.tab_bytes);  // MODE_GROUP_LDS: n[G] when counting, then the cells
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ns = p.num_slots;
  const int64_t G = p.num_groups;
  const bool tab_lds = p.tab_lds != 0;
  const bool counting = p.n != nullptr;
  u64* lds_cells = lds_n + (MODE == MODE_GROUP_LDS && counting ? G : 0);

  if (MODE == MODE_GROUP_LDS) {
    const int64_t words = G * ns + (counting ? G : 0);
    for (int64_t i = threadIdx.x; i < words; i += kBlock) lds_n[i] = 0ull;
    __syncthreads();
  }

  // MODE_AGG: the lane's best key per slot
  u64 best[MODE == MODE_AGG ? kWMaxSlots : 1];
#pragma unroll
  for (int s = 0; s < (MODE == MODE_AGG ? kWMaxSlots : 1); ++s) best[s] = 0ull;

  // hi_of[id] of slot s in segment S (an unmatched lane reads entry 0, always there)
  auto hi_of = [&](int s, WSegPtr S, bool hit, uint32_t id) -> uint32_t {
    const uint32_t at = hit ? min(id, (uint32_t)(S->card[s] - 1)) : 0u;
    return tab_lds ? lds_tab[p.tab_off[s] + at] : gld(S->hi_of[s] + at);
  };

  int32_t staged = -1;  // the segment whose hi_of tables are in LDS
  for (int c = p.chunk_begin + (int)blockIdx.x; c < p.chunk_end; c += (int)gridDim.x) {
    const PH_CONST Chunk* ck = (const PH_CONST Chunk*)p.chunks + c;  // C-style cast = addrspacecast
    const int32_t seg = ck->seg, wb = ck->word_begin, we = ck->word_end;
    WSegPtr S = (WSegPtr)p.segs + seg;
    const int32_t nd = S->num_docs;
    const uint32_t lo_base = S->lo_base;
    const u64* mask = S->mask;
    if (tab_lds && seg != staged) {  // (workgroup-uniform: every wave walks the same chunks)
      __syncthreads();
#pragma unroll
      for (int s = 0; s < kWMaxSlots; ++s)
        if (s < ns) {
          const uint32_t* src = S->hi_of[s];
          const int32_t room = (s + 1 < ns ? p.tab_off[s + 1] : p.tab_bytes / 4) - p.tab_off[s];
          const int32_t n = min(S->card[s], room);
          for (int32_t i = threadIdx.x; i < n; i += kBlock) lds_tab[p.tab_off[s] + i] = gld(src + i);
        }
      __syncthreads();
      staged = seg;
    }
    u64 pc = 0ull;  // REG: per lane, else wave-uniform: matched docs of the chunk

    if constexpr (REG) {
      constexpr int C = 4;  // a lane's dwords of a stream of at most 16 bits: four 16-byte registers
      for (int32_t w0 = wb + wave * kRegTileWords; w0 < we; w0 += kWaves * kRegTileWords) {
        const int32_t nw = min(kRegTileWords, we - w0);
        const int32_t ndoc = max(0, min(nw * 64, nd - w0 * 64));
        const int32_t nv = max(0, min(32, ndoc - lane * 32));
        uint32_t m = nv >= 32 ? 0xffffffffu : ((1u << nv) - 1u);
        if (mask && nv > 0) m &= (uint32_t)(gld(mask + w0 + (lane >> 1)) >> ((lane & 1) * 32));
        if (!__ballot(m != 0u)) continue;
        pc += (u64)__builtin_popcount(m);
        const uint32_t lo0 = lo_base + (uint32_t)w0 * 64u + (uint32_t)lane * 32u;
        // (the slot loop is unrolled so that every index into the by-value parameter arrays is static)
#pragma unroll
        for (int s = 0; s < kWMaxSlots; ++s) {
          if (s < ns) {
            const int32_t vb = S->tbits[s];
            u32x4 pool[C];
            uint32_t ids[32];
            reg_load<C>(true, lane * 32 < ndoc, S->tfwd[s], vb, ((int64_t)nd * vb + 7) / 8, w0 * 2, lane, pool);
            reg_unpack<C>(pool, vb, ids);
            uint32_t bh = 0u, bj = 0u;  // the run's keys ascend with j: the last doc with the largest hi
#pragma unroll
            for (int j = 0; j < 32; ++j) {
              const bool hit = (m >> j) & 1u;
              const uint32_t h = hi_of(s, S, hit, ids[j]);
              const bool take = hit && h >= bh;
              bh = take ? h : bh;
              bj = take ? (uint32_t)j : bj;
            }
            const u64 k = bh ? (((u64)bh << 32) | (u64)(lo0 + bj)) : 0ull;
            best[MODE == MODE_AGG ? s : 0] = max(best[MODE == MODE_AGG ? s : 0], k);
          }
        }
      }
      pc = (u64)wave_sum_i64((int64_t)pc);
    } else {
      for (int32_t w = wb + wave; w < we; w += kWaves) {
        const int32_t left = nd - w * 64;
        if (left <= 0) break;
        u64 m = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
        if (mask) m &= gld(mask + w);
        if (m == 0ull) continue;
        pc += (u64)__popcll(m);
        bool hit = (m >> lane) & 1ull;
        const uint32_t doc = (uint32_t)w * 64u + (uint32_t)lane;
        int64_t key = 0;
        if (MODE != MODE_AGG) {
          if (hit) {
#pragma unroll
            for (int g = 0; g < kMaxGroupCols; ++g) {
              if (g < p.num_group_cols) {
                uint32_t id = unpack_bits(S->gfwd[g], S->gbits[g], doc);
                const int32_t* rm = S->gremap[g];
                if (rm) id = (uint32_t)gld(rm + id);
                key += (int64_t)id * p.group_stride[g];
              }
            }
            if (key < 0 || key >= G) hit = false;  // (never: remapped ids index the call's dictionaries)
          }
          if (!hit) key = 0;
          if (counting)
            w_match_count(MODE == MODE_GROUP_LDS ? lds_n : p.n, key, hit, lane, MODE == MODE_GROUP_GLOBAL, p.combine_rounds);
        }
#pragma unroll
        for (int s = 0; s < kWMaxSlots; ++s) {
          if (s < ns) {
            const uint32_t id = hit ? unpack_bits(S->tfwd[s], S->tbits[s], doc) : 0u;
            const u64 k = hit ? (((u64)hi_of(s, S, hit, id) << 32) | (u64)(lo_base + doc)) : 0ull;
            if (MODE == MODE_AGG) {
              best[MODE == MODE_AGG ? s : 0] = max(best[MODE == MODE_AGG ? s : 0], k);
            } else {
              u64* table = MODE == MODE_GROUP_LDS ? lds_cells : p.cells;
              const int64_t cell = key * ns + s;
              const bool pass = hit && k > w_peek(table + cell, MODE == MODE_GROUP_GLOBAL);  // the screen
              w_match_max(table, cell, k, pass, lane, MODE == MODE_GROUP_GLOBAL, p.combine_rounds);
            }
          }
        }
      }
    }
    if (lane == 0 && pc) {
      atomicAdd(p.seg_count + seg, pc);
      if (MODE == MODE_AGG && counting) atomicAdd(p.n, pc);
    }
  }

  if constexpr (MODE == MODE_AGG) {
    // a wave maximum by shuffles, one LDS cell per wave and slot, one HBM atomic per workgroup and slot
    u64* lds_best = lds_n;
#pragma unroll
    for (int s = 0; s < kWMaxSlots; ++s) {
      if (s < ns) {
        const u64 v = wave_max_u64(best[s]);
        if (lane == 0) lds_best[wave * kWMaxSlots + s] = v;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < ns) {
      u64 v = 0ull;
#pragma unroll
      for (int k = 0; k < kWaves; ++k) v = max(v, lds_best[k * kWMaxSlots + (int)threadIdx.x]);
      if (v && v > w_peek(p.cells + threadIdx.x, true)) w_max(p.cells + threadIdx.x, v, true);
    }
  } else if constexpr (MODE == MODE_GROUP_LDS) {
    __syncthreads();
    if (counting)
      for (int64_t g = threadIdx.x; g < G; g += kBlock) {
        const u64 docs = lds_n[g];
        if (docs) atomicAdd(p.n + g, docs);
      }
    for (int64_t i = threadIdx.x; i < G * ns; i += kBlock) {
      const u64 v = lds_cells[i];
      if (v && v > w_peek(p.cells + i, true)) w_max(p.cells + i, v, true);
    }
  }
}

// ---- finish: cells -> (value, time) pairs
__global__ void __launch_bounds__(256) k_withtime_finish(const WFinishParams p) {
  const int64_t total = p.num_groups * p.num_aggs;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int a = (int)(i / p.num_groups);
    const int64_t g = i - (int64_t)a * p.num_groups;
    const WFinAgg* A = p.aggs + a;
    const int slot = gld(&A->slot);
    const u64 cell = gld(p.cells + g * p.num_slots + slot);
    if (a == 0 && p.write_n) p.n[g] = gld(p.cells + g * p.num_slots) != 0ull;
    int64_t value = gld(&A->default_value), time = gld(&A->default_time);
    if (cell) {
      const uint32_t ord = 0xFFFFFFFFu - (uint32_t)cell;
      int lo = 0, hi = p.num_segs - 1;  // the last segment whose base is at most ord
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (gld(&p.segs[mid].base) <= ord) lo = mid;
        else hi = mid - 1;
      }
      const WFinSeg* S = p.segs + lo;
      const int32_t nd = gld(&S->num_docs);
      const int64_t doc = (int64_t)nd - 1 - (int64_t)(ord - gld(&S->base));
      const int64_t T = gld(&A->num_times);
      const int64_t h = (int64_t)(cell >> 32);
      const int64_t rank = gld(&A->first) ? T - h : h - 1;
      if (doc >= 0 && doc < nd && rank >= 0 && rank < T) {  // (always: the scan wrote the cell from such a doc)
        uint32_t id = unpack_bits(gld(&S->dfwd[a]), gld(&S->dbits[a]), (uint32_t)doc);
        id = min(id, (uint32_t)(gld(&S->dcard[a]) - 1));
        const void* vals = gld(&S->dvals[a]);
        double d = 0.0;
        const int kind = gld(&S->dkind[a]);
        if (kind == WT_I64) value = gld(static_cast<const int64_t*>(vals) + id);
        else if (kind == WT_F64_OF_I64) d = (double)gld(static_cast<const int64_t*>(vals) + id);
        else if (kind == WT_F64) d = gld(static_cast<const double*>(vals) + id);
        else d = (double)(float)gld(static_cast<const double*>(vals) + id);
        if (kind != WT_I64) value = __double_as_longlong(d);
        time = gld(gld(&A->time_of_rank) + rank);
      }
    }
    int64_t* out = gld(&A->out) + 2 * g;
    out[0] = value;
    out[1] = time;
  }
}

size_t withtime_lds_bytes(const WParams& p, int mode) {
  size_t cells = 0;
  if (mode == MODE_AGG) cells = (size_t)kWaves * kWMaxSlots;
  else if (mode == MODE_GROUP_LDS) cells = (size_t)p.num_groups * ((size_t)p.num_slots + (p.n ? 1 : 0));
  return (size_t)p.tab_bytes + 8 * cells;
}

template <int MODE, int REG>
static void launch_form(const WParams& p, int grid, size_t lds, hipStream_t s) {
  allow_lds(k_scan_withtime<MODE, REG>, lds);
  hipLaunchKernelGGL((k_scan_withtime<MODE, REG>), dim3(grid), dim3(kBlock), lds, s, p);
}

void launch_scan_withtime(const WParams& p, int mode, bool reg, int grid, hipStream_t s) {
  if (!p.segs || !p.chunks || !p.cells || !p.seg_count || p.num_slots <= 0 || p.num_slots > kWMaxSlots ||
      p.num_group_cols < 0 || p.num_group_cols > kMaxGroupCols || p.num_groups <= 0 || p.tab_bytes < 0 ||
      (p.tab_bytes & 15) || p.combine_rounds < 0 || grid <= 0 || (reg && mode != MODE_AGG))
    fail(PH_ERR_INVALID_ARGUMENT, "with-time scan with bad parameters");
  for (int i = 0; i < p.num_slots; ++i)
    if (p.tab_off[i] < 0 || (p.tab_lds && 4 * p.tab_off[i] > p.tab_bytes))
      fail(PH_ERR_INVALID_ARGUMENT, "with-time scan with a bad slot");
  const size_t lds = withtime_lds_bytes(p, mode);
  if (lds > 160 * 1024) fail(PH_ERR_INVALID_ARGUMENT, "with-time scan tables exceed the LDS of one CU");
  switch (mode) {
    case MODE_AGG:
      if (reg) launch_form<MODE_AGG, 1>(p, grid, lds, s);
      else launch_form<MODE_AGG, 0>(p, grid, lds, s);
      break;
    case MODE_GROUP_LDS: launch_form<MODE_GROUP_LDS, 0>(p, grid, lds, s); break;
    case MODE_GROUP_GLOBAL: launch_form<MODE_GROUP_GLOBAL, 0>(p, grid, lds, s); break;
    default: fail(PH_ERR_UNSUPPORTED, "with-time functions in this plan mode");
  }
  PH_HIP_CHECK(hipGetLastError());
}

void launch_withtime_finish(const WFinishParams& p, hipStream_t s) {
  if (p.num_groups <= 0 || p.num_aggs <= 0 || p.num_aggs > kMaxAggs || p.num_slots <= 0 || p.num_slots > kWMaxSlots ||
      p.num_segs <= 0 || !p.cells || !p.n || !p.segs || !p.aggs)
    fail(PH_ERR_INVALID_ARGUMENT, "with-time finish with bad parameters");
  const int64_t blocks = (p.num_groups * p.num_aggs + 255) / 256;
  hipLaunchKernelGGL(k_withtime_finish, dim3((unsigned)std::min<int64_t>(blocks, 1 << 20)), dim3(256), 0, s, p);
  PH_HIP_CHECK(hipGetLastError());
}

}  // namespace ph
