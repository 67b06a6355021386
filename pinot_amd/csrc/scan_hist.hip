// scan_hist.hip -- exact PERCENTILE on the generic scan.
//
// The reference appends every matched value to a DoubleArrayList per result holder, sorts it at the end and returns
// element (int)((long) size * percentile / 100) (PercentileAggregationFunction.java:77-94, 146-158).  Here a result row
// holds one histogram per PERCENTILE slot (a distinct column) over the slot's result dictionary -- the sorted value
// union of the column over the queried segments, or the table dictionary -- so the rows of different segments add up,
// the element of a rank is a prefix sum away and one histogram serves every percentile of its column.
//
//   k_scan<.., LATE = 4>   the generic scan; for every matched doc and slot, id = remap ? remap[dictId] : dictId and
//                          counter hist_off[h] + id of the row is incremented (scan_kernel.h hist_insert): in the
//                          workgroup's LDS table (MODE_AGG when it fits, MODE_GROUP_LDS), flushed counter by counter
//                          at the end, or straight in the HBM table (MODE_AGG otherwise, MODE_GROUP_GLOBAL) after
//                          the lanes of a wave that hold the same counter have been combined.  It carries the
//                          DISTINCTCOUNT insert of LATE = 3 too (num_dc may be 0), so that mixed queries work.
//   k_percentile_finish    right after it on the same stream: one wave per (row, slot) histogram.  The lanes stride
//                          over its counters, a wave reduction gives n (and the largest present id); for each
//                          aggregation of the slot the rank is computed in double as Java does, and a wave prefix
//                          scan over 64-counter chunks finds the smallest id whose cumulative count exceeds it
//                          (whole 4096-counter tiles before the rank's are skipped with one reduction each).
//                          Lane 0 stores that dictId (-1 for n = 0); the host maps it to the dictionary's value.
//
// Only PERCENTILE queries instantiate LATE = 4, over the general value-column variant (REC64 = 0).
#include <algorithm>

#include "scan_kernel.h"

namespace ph {

__global__ void __launch_bounds__(kBlock) k_percentile_finish(const PctFinishParams f) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * kBlock + threadIdx.x) >> 6));
  const int64_t nwaves = (int64_t)gridDim.x * kWaves;
  const int64_t total = f.rows * f.num_slots;
  for (int64_t e = wave; e < total; e += nwaves) {
    const int64_t g = e / f.num_slots;
    const int h = (int)(e - g * f.num_slots);
    const uint32_t* row = f.hist + g * f.row_words + f.off[h];
    const int32_t d = f.size[h];
    int64_t n = 0, last = -1;  // the row's total and its largest present id
    for (int32_t i = lane; i < d; i += 64) {
      const uint32_t c = gld(row + i);
      n += c;
      if (c) last = i;
    }
    n = wave_sum_i64(n);
    last = wave_max_i64(last);
    for (int a = 0; a < f.num_aggs; ++a) {
      if (f.agg_slot[a] != h) continue;
      int32_t id = -1;
      if (n > 0) {
        const double pct = f.agg_p[a];
        if (pct == 100.0) {
          id = (int32_t)last;
        } else {
          // (int) ((long) size * _percentile / 100): double arithmetic, truncated; below n for every p < 100
          int64_t rank = (int64_t)((double)n * pct / 100.0);
          rank = rank > n - 1 ? n - 1 : (rank < 0 ? 0 : rank);
          int64_t base = 0;  // docs of the counters before this chunk
          int32_t c0 = 0;
          // coarse steps first: whole tiles of 64 chunks, one wave reduction each (64 independent coalesced loads per
          // lane), until the tile that holds the rank; the chunk loop below then searches that tile, or the tail
          constexpr int32_t kTile = 64 * 64;
          for (; c0 + kTile <= d; c0 += kTile) {
            int64_t s = 0;
#pragma unroll 8
            for (int32_t j = 0; j < 64; ++j) s += gld(row + c0 + j * 64 + lane);
            s = wave_sum_i64(s);
            if (base + s > rank) break;
            base += s;
          }
          for (; c0 < d; c0 += 64) {
            const int32_t i = c0 + lane;
            int64_t incl = i < d ? (int64_t)gld(row + i) : 0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {  // inclusive prefix sum over the wave
              const int64_t t = __shfl_up(incl, o, 64);
              if (lane >= o) incl += t;
            }
            const unsigned long long past = __ballot(base + incl > rank);
            if (past) {
              id = c0 + (__ffsll((long long)past) - 1);
              break;
            }
            base += __shfl(incl, 63, 64);
          }
        }
      }
      if (lane == 0) f.ids[g * f.num_aggs + a] = id;
    }
  }
}

void launch_percentile_finish(const PctFinishParams& f, hipStream_t s) {
  if (!f.hist || !f.ids || f.num_slots <= 0 || f.num_slots > kMaxHll || f.num_aggs <= 0 || f.num_aggs > kMaxAggs ||
      f.rows <= 0)
    fail(PH_ERR_INVALID_ARGUMENT, "percentile finish without a table");
  const int64_t n = f.rows * f.num_slots;
  const uint32_t blocks = (uint32_t)std::max<int64_t>(1, std::min<int64_t>((n + kWaves - 1) / kWaves, 4096));
  hipLaunchKernelGGL(k_percentile_finish, dim3(blocks), dim3(kBlock), 0, s, f);
  PH_HIP_CHECK(hipGetLastError());
}

template <int MODE, int NG>
static void launch_hist_scan(const KParams& p, int grid, size_t lds, hipStream_t s) {
  allow_lds(k_scan<MODE, NG, 0, 4>, lds);
  hipLaunchKernelGGL((k_scan<MODE, NG, 0, 4>), dim3(grid), dim3(kBlock), lds, s, p);
}

template <int MODE>
static void launch_hist_ng(const KParams& p, int ng, int grid, size_t lds, hipStream_t s) {
  switch (ng) {
    case 1: launch_hist_scan<MODE, 1>(p, grid, lds, s); break;
    case 2: launch_hist_scan<MODE, 2>(p, grid, lds, s); break;
    case 3: launch_hist_scan<MODE, 3>(p, grid, lds, s); break;
    default: launch_hist_scan<MODE, 4>(p, grid, lds, s); break;
  }
}

void launch_scan_hist(const KParams& p, int mode, int ng, int grid, size_t lds, hipStream_t s) {
  if (!p.out_hist || p.num_hist <= 0 || p.num_hist > kMaxHll || p.hist_row_words <= 0)
    fail(PH_ERR_INVALID_ARGUMENT, "PERCENTILE scan without a histogram table");
  if (p.num_dc && (!p.out_dc || p.num_dc > kMaxHll || p.dc_row_words <= 0))
    fail(PH_ERR_INVALID_ARGUMENT, "DISTINCTCOUNT scan without a bitset table");
  switch (mode) {
    case MODE_AGG: launch_hist_scan<MODE_AGG, 0>(p, grid, lds, s); break;
    case MODE_GROUP_LDS: launch_hist_ng<MODE_GROUP_LDS>(p, ng, grid, lds, s); break;
    case MODE_GROUP_GLOBAL: launch_hist_ng<MODE_GROUP_GLOBAL>(p, ng, grid, lds, s); break;
    default: fail(PH_ERR_UNSUPPORTED, "PERCENTILE in this plan mode");
  }
  PH_HIP_CHECK(hipGetLastError());
}

}  // namespace ph
