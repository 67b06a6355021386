// scan_bins.hip -- HISTOGRAM(col, lower, upper, numBins) / HISTOGRAM(col, ARRAY[e0, ..., eB]): bin counts per result row.
//
// The reference keeps a DoubleArrayList of B counts per result holder and adds 1.0 at getBinId(value) per doc
// (HistogramAggregationFunction.java:117-141, 191-298).  The bin depends on the doc's dictionary value only, so the
// planner (bins.cpp) evaluates getBinId once per dictionary entry on the host and the scan reads bin_of[dictId], a uint16
// table per (segment, slot) in which B stands for "outside every bin".
//
// Row layout.  A slot is one (column, bins) pair.  A row holds, per slot, B + 1 uint32 cells: cell b counts the matched
// docs of bin b, cell B those outside every bin.  The cells of any slot therefore add up to the row's matched docs: that
// total is the row's existence test and its COUNT(*), so there is no n[G] table in the scan.  Row g of the HBM table is
// cells [g row_cells, (g + 1) row_cells), slot s at cell_off[s].  A call holds fewer than 2^32 docs (the planner
// refuses more), so no cell wraps.
//
// Bin tables.  When the tables of every slot fit BParams::tab_bytes (the planner's budget, the context option
// bins_table_lds_max) a workgroup stages the current segment's tables into LDS -- at its first chunk and again when its
// chunk loop reaches another segment, between two barriers -- and a doc's lookup is one ds_read_u16; otherwise the
// lookup is a gather from HBM (gld: the tables are dictionary-sized and L2-resident).
//
// Contention.  A histogram is the opposite of a group-by table: nearly every doc of a wave lands on a handful of
// cells.  So the 64 docs a wave handles together are combined before anything is added:
//   ballot form (MODE_AGG, a slot of at most kBBallotCells cells): for every cell c one __ballot of the lanes whose doc
//     has it; lane c adds the popcount to a register.  No LDS traffic in the loop at all; the cost is one ballot per
//     cell and step whatever the data, which is why it ends at kBBallotCells.
//   match form (everything else): the first lane still owing its add broadcasts its cell (readfirstlane), a __ballot
//     finds the lanes with the same cell, the first of them adds the popcount, all of them retire.  After
//     kBMatchRounds rounds the lanes left add 1 each, so a wave whose docs spread over many cells costs a bounded
//     number of rounds plus one atomic instruction.
// kBMatchRounds = 4 comes from counting instructions (a ballot step is ~3 scalar-side instructions per cell, a match
// round ~8 plus an LDS add) and is unmeasured.  kBBallotCells = 8: the count put the crossover at 16 cells, but a build
// with 16 ran the ballot form level with the match form at 11 cells and 12 % behind it at 16 (single measurements,
// DESIGN.md, "Histogram bins"), so the ballot form is kept where it should still win; the exact crossover is unmeasured.
//
//   MODE_AGG           each of the four waves owns a private copy of the row in LDS (row_cells x 4 bytes: at B = 1024 and
//                      4 slots 16.4 KB, 65.6 KB for the workgroup); the leader's add is a plain LDS atomic on the wave's
//                      own copy.  The copies are summed once per workgroup, then one HBM atomic per non-zero cell.
//   MODE_GROUP_LDS     one workgroup-shared table of G x row_cells cells; lanes with equal (key, bin) combine by the
//                      match form before the LDS atomic; flushed at the end, zero cells skipped.
//   MODE_GROUP_GLOBAL  the same combining, then atomicAdd straight into the HBM table.
//
// Decode.  k_scan_bins<MODE_AGG, REG = 1>: register-direct (reg_decode.h), for launches in which every slot's packed
// width is at most 16 bits: a wave takes 2048-doc tiles of a chunk, lane l owns docs [32 l, 32 l + 32) of the tile and
// its 32 mask bits are half l % 2 of bitmap word l / 2; a tile whose masks are zero across the wave issues no load.
// Step j of a tile handles doc j of every lane's run, 64 docs together, with the combining above.  REG = 0 (wider
// columns, and every group-by mode): workgroups stride over chunks, waves over 64-doc mask words, lane l owns doc
// 64 w + l, decoded per doc by unpack_bits; all-zero words are skipped.
//
// k_bins_finish: one wave per (row, slot) reads the slot's B + 1 cells, sums them by shuffles (slot 0's sum is the
// row's matched docs) and writes the B counts as doubles.  All stores are plain vector stores; no inline assembly.
#include <algorithm>

#include "reg_decode.h"

namespace ph {

typedef const PH_CONST BSegment* BSegPtr;
typedef unsigned long long u64;

// *cell += v on an LDS or an HBM cell, result unused
__device__ __forceinline__ void b_add(uint32_t* cell, uint32_t v, bool hbm) {
  if (hbm) (void)__hip_atomic_fetch_add(cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else (void)__hip_atomic_fetch_add(cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// match form: the active lanes (`mine`) add 1 to table[cell]; lanes with equal cells are combined first.  Called by
// every lane of the wave (the loop's trip count is wave-uniform)
__device__ __forceinline__ void b_match_add(uint32_t* table, int64_t cell, bool mine, int lane, bool hbm) {
#pragma unroll 1
  for (int round = 0; round < kBMatchRounds; ++round) {
    if (!__ballot(mine)) return;
    if (mine) {
      const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)cell);
      const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((u64)cell >> 32));
      const bool same = cell == (int64_t)(((u64)hi << 32) | lo);
      const u64 peers = __ballot(same);  // (of the lanes still owing: the branch masks the others)
      if (same) {
        if (lane == __ffsll((long long)peers) - 1) b_add(table + cell, (uint32_t)__popcll(peers), hbm);
        mine = false;
      }
    }
  }
  if (mine) b_add(table + cell, 1u, hbm);
}

template <int MODE, int REG>
__global__ void __launch_bounds__(kBlock) k_scan_bins(const BParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char b_lds[];
  uint16_t* lds_tab = reinterpret_cast<uint16_t*>(b_lds);
  uint32_t* lds_cnt = reinterpret_cast<uint32_t*>(b_lds + p.tab_bytes);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ns = p.num_slots;
  const int rc = p.row_cells;
  const int64_t G = p.num_groups;
  const bool tab_lds = p.tab_lds != 0;

  // the LDS counters: MODE_AGG a copy of the row per wave, MODE_GROUP_LDS the workgroup's G rows
  const int64_t lds_cells = MODE == MODE_AGG ? (int64_t)kWaves * rc : (MODE == MODE_GROUP_LDS ? G * rc : 0);
  for (int64_t i = threadIdx.x; i < lds_cells; i += kBlock) lds_cnt[i] = 0u;
  uint32_t* const my_cnt = lds_cnt + (MODE == MODE_AGG ? wave * rc : 0);
  __syncthreads();

  // ballot form: lane c's count of cell c of slot s (MODE_AGG only)
  uint32_t bal_acc[MODE == MODE_AGG ? kBMaxSlots : 1];
#pragma unroll
  for (int s = 0; s < (MODE == MODE_AGG ? kBMaxSlots : 1); ++s) bal_acc[s] = 0u;

  // one step of one slot: 64 docs, lane's doc `hit` or not with dictId `id` and dense key `key`
  auto count = [&](int s, BSegPtr S, bool hit, uint32_t id, int64_t key) {
    const int B = p.bins[s];
    uint32_t bin;  // (an unmatched lane reads entry 0, always there, and adds nothing)
    if (tab_lds) bin = lds_tab[p.tab_off[s] + (hit ? id : 0u)];
    else bin = gld(S->bin_of[s] + (hit ? id : 0u));
    bin = min(bin, (uint32_t)B);
    if (MODE == MODE_AGG && B + 1 <= kBBallotCells) {
      uint32_t mine = 0u;
#pragma unroll 1
      for (int c = 0; c <= B; ++c) {
        const uint32_t n = (uint32_t)__popcll(__ballot(hit && bin == (uint32_t)c));
        mine = lane == c ? n : mine;
      }
      bal_acc[MODE == MODE_AGG ? s : 0] += mine;
    } else if (MODE == MODE_GROUP_GLOBAL) {
      b_match_add(p.cells, key * rc + p.cell_off[s] + bin, hit, lane, true);
    } else {
      b_match_add(my_cnt, key * rc + p.cell_off[s] + bin, hit, lane, false);
    }
  };

  int32_t staged = -1;  // the segment whose bin tables are in LDS
  for (int c = p.chunk_begin + (int)blockIdx.x; c < p.chunk_end; c += (int)gridDim.x) {
    const PH_CONST Chunk* ck = (const PH_CONST Chunk*)p.chunks + c;  // C-style cast = addrspacecast
    const int32_t seg = ck->seg, wb = ck->word_begin, we = ck->word_end;
    BSegPtr S = (BSegPtr)p.segs + seg;
    const int32_t nd = S->num_docs;
    const u64* mask = S->mask;
    if (tab_lds && seg != staged) {  // (workgroup-uniform: every wave walks the same chunks)
      __syncthreads();
#pragma unroll
      for (int s = 0; s < kBMaxSlots; ++s)
        if (s < ns) {
          const uint16_t* src = S->bin_of[s];
          const int32_t room = ((s + 1 < ns ? p.tab_off[s + 1] : p.tab_bytes / 2) - p.tab_off[s]);
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
        // (the slot loop is unrolled so that every index into the by-value parameter arrays is static)
#pragma unroll
        for (int s = 0; s < kBMaxSlots; ++s) {
          if (s < ns) {
            const int32_t vb = S->vbits[s];
            u32x4 pool[C];
            uint32_t ids[32];
            reg_load<C>(true, lane * 32 < ndoc, S->vfwd[s], vb, ((int64_t)nd * vb + 7) / 8, w0 * 2, lane, pool);
            reg_unpack<C>(pool, vb, ids);
#pragma unroll
            for (int j = 0; j < 32; ++j) count(s, S, (m >> j) & 1u, ids[j], 0);
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
        if (MODE != MODE_AGG && hit) {
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
#pragma unroll
        for (int s = 0; s < kBMaxSlots; ++s) {
          if (s < ns) {
            const uint32_t id = hit ? unpack_bits(S->vfwd[s], S->vbits[s], doc) : 0u;
            count(s, S, hit, id, hit ? key : 0);
          }
        }
      }
    }
    if (lane == 0 && pc) atomicAdd(p.seg_count + seg, pc);
  }

  if constexpr (MODE == MODE_AGG) {
    // the ballot-form registers join the wave's copy, the four copies are summed, one HBM atomic per non-zero cell
#pragma unroll
    for (int s = 0; s < kBMaxSlots; ++s)
      if (s < ns && p.bins[s] + 1 <= kBBallotCells && lane <= p.bins[s]) my_cnt[p.cell_off[s] + lane] = bal_acc[s];
    __syncthreads();
    for (int i = threadIdx.x; i < rc; i += kBlock) {
      uint32_t v = 0u;
#pragma unroll
      for (int k = 0; k < kWaves; ++k) v += lds_cnt[k * rc + i];
      if (v) b_add(p.cells + i, v, true);
    }
  } else if constexpr (MODE == MODE_GROUP_LDS) {
    __syncthreads();
    for (int64_t i = threadIdx.x; i < G * rc; i += kBlock) {
      const uint32_t v = lds_cnt[i];
      if (v) b_add(p.cells + i, v, true);
    }
  }
}

// ---- finish: cells -> (n, the B counts as doubles)
__global__ void __launch_bounds__(256) k_bins_finish(const BFinishParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4, total = p.num_groups * p.num_slots;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < total; i += waves) {
    const int sl = (int)(i / p.num_groups);
    const int64_t g = i - (int64_t)sl * p.num_groups;
    // (static indices into the by-value parameter arrays: a dynamic one would copy them to scratch)
    int B = 0, off = 0;
    double* dst = nullptr;
#pragma unroll
    for (int k = 0; k < kBMaxSlots; ++k)
      if (k == sl) {
        B = p.bins[k];
        off = p.cell_off[k];
        dst = p.out[k];
      }
    const uint32_t* row = p.cells + g * p.row_cells + off;
    u64 sum = 0ull;
    for (int b = lane; b <= B; b += 64) {
      const uint32_t v = gld(row + b);
      sum += v;
      if (b < B) dst[g * B + b] = (double)v;
    }
    sum = (u64)wave_sum_i64((int64_t)sum);
    if (sl == 0 && lane == 0) p.n[g] = sum;
  }
}

size_t bins_lds_bytes(const BParams& p, int mode) {
  size_t cells = 0;
  if (mode == MODE_AGG) cells = (size_t)kWaves * (size_t)p.row_cells;
  else if (mode == MODE_GROUP_LDS) cells = (size_t)p.num_groups * (size_t)p.row_cells;
  return (size_t)p.tab_bytes + 4 * cells;
}

template <int MODE, int REG>
static void launch_form(const BParams& p, int grid, size_t lds, hipStream_t s) {
  allow_lds(k_scan_bins<MODE, REG>, lds);
  hipLaunchKernelGGL((k_scan_bins<MODE, REG>), dim3(grid), dim3(kBlock), lds, s, p);
}

void launch_scan_bins(const BParams& p, int mode, bool reg, int grid, hipStream_t s) {
  if (!p.segs || !p.chunks || !p.cells || !p.seg_count || p.num_slots <= 0 || p.num_slots > kBMaxSlots ||
      p.num_group_cols < 0 || p.num_group_cols > kMaxGroupCols || p.num_groups <= 0 || p.row_cells <= 0 ||
      p.tab_bytes < 0 || (p.tab_bytes & 15) || grid <= 0)
    fail(PH_ERR_INVALID_ARGUMENT, "histogram scan with bad parameters");
  int cells = 0;
  for (int i = 0; i < p.num_slots; ++i) {
    if (p.bins[i] < 1 || p.bins[i] > kBMaxBins || p.cell_off[i] != cells || p.tab_off[i] < 0 ||
        (p.tab_lds && 2 * p.tab_off[i] > p.tab_bytes))
      fail(PH_ERR_INVALID_ARGUMENT, "histogram scan with a bad slot");
    cells += p.bins[i] + 1;
  }
  if (cells != p.row_cells || (reg && mode != MODE_AGG))
    fail(PH_ERR_INVALID_ARGUMENT, "histogram scan with a bad row layout");
  const size_t lds = bins_lds_bytes(p, mode);
  if (lds > 160 * 1024) fail(PH_ERR_INVALID_ARGUMENT, "histogram scan tables exceed the LDS of one CU");
  switch (mode) {
    case MODE_AGG:
      if (reg) launch_form<MODE_AGG, 1>(p, grid, lds, s);
      else launch_form<MODE_AGG, 0>(p, grid, lds, s);
      break;
    case MODE_GROUP_LDS: launch_form<MODE_GROUP_LDS, 0>(p, grid, lds, s); break;
    case MODE_GROUP_GLOBAL: launch_form<MODE_GROUP_GLOBAL, 0>(p, grid, lds, s); break;
    default: fail(PH_ERR_UNSUPPORTED, "histograms in this plan mode");
  }
  PH_HIP_CHECK(hipGetLastError());
}

void launch_bins_finish(const BFinishParams& p, hipStream_t s) {
  if (p.num_groups <= 0 || p.num_slots <= 0 || p.num_slots > kBMaxSlots || !p.n || !p.cells)
    fail(PH_ERR_INVALID_ARGUMENT, "histogram finish with bad parameters");
  const int64_t blocks = (p.num_groups * p.num_slots + 3) / 4;
  hipLaunchKernelGGL(k_bins_finish, dim3((unsigned)std::min<int64_t>(blocks, 1 << 20)), dim3(256), 0, s, p);
  PH_HIP_CHECK(hipGetLastError());
}

}  // namespace ph
