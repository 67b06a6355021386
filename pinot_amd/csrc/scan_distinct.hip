// scan_distinct.hip -- exact DISTINCTCOUNT on the generic scan.
//
// The reference aggregates DISTINCTCOUNT over a dictionary column in dictId space: a RoaringBitmap of dictIds per
// result holder (BaseDistinctAggregateAggregationFunction.java:133-168), turned into a value set only when the result
// is extracted (:77-108); the final result is the set's size (DistinctCountAggregationFunction.java:61-68).  Here a
// result row holds one bitset per DISTINCTCOUNT slot over the slot's result dictionary (the sorted value union of the
// column over the queried segments, or the table dictionary), so the rows of different segments OR together.
//
//   k_scan<.., LATE = 3>   the generic scan; for every matched doc and slot, id = remap ? remap[dictId] : dictId and
//                          bit id & 31 of word id >> 5 of the row's slot is ORed in (scan_kernel.h distinct_insert): in
//                          the workgroup's LDS table (MODE_AGG when it fits, MODE_GROUP_LDS), flushed word by word at
//                          the end, or straight in the HBM table (MODE_AGG otherwise, MODE_GROUP_GLOBAL)
//   k_distinct_finish      right after it on the same stream: one wave per (row, slot) bitset, the lanes stride over
//                          its words, __popc, a wave reduction, lane 0 stores the int32 count
//
// Only DISTINCTCOUNT queries instantiate LATE = 3, over the general value-column variant (REC64 = 0).
#include <algorithm>

#include "scan_kernel.h"

namespace ph {

__global__ void __launch_bounds__(kBlock) k_distinct_finish(const KParams p, const int64_t rows) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * kBlock + threadIdx.x) >> 6));
  const int64_t nwaves = (int64_t)gridDim.x * kWaves;
  const int64_t n = rows * p.num_dc;
  for (int64_t e = wave; e < n; e += nwaves) {
    const int64_t g = e / p.num_dc;
    const int h = (int)(e - g * p.num_dc);
    const uint32_t* row = p.out_dc + g * p.dc_row_words + p.dc_off[h];
    const int32_t words = p.dc_words[h];
    int64_t c = 0;
    for (int32_t w = lane; w < words; w += 64) c += __popc(gld(row + w));  // W == 1: lane 0 alone reads
    c = wave_sum_i64(c);
    if (lane == 0) p.dc_counts[e] = (int32_t)c;
  }
}

void launch_distinct_finish(const KParams& p, int64_t rows, hipStream_t s) {
  if (!p.out_dc || !p.dc_counts || p.num_dc <= 0 || rows <= 0) fail(PH_ERR_INVALID_ARGUMENT, "distinct finish without a table");
  const int64_t n = rows * p.num_dc;
  const uint32_t blocks = (uint32_t)std::max<int64_t>(1, std::min<int64_t>((n + kWaves - 1) / kWaves, 4096));
  hipLaunchKernelGGL(k_distinct_finish, dim3(blocks), dim3(kBlock), 0, s, p, rows);
  PH_HIP_CHECK(hipGetLastError());
}

template <int MODE, int NG>
static void launch_distinct_scan(const KParams& p, int grid, size_t lds, hipStream_t s) {
  allow_lds(k_scan<MODE, NG, 0, 3>, lds);
  hipLaunchKernelGGL((k_scan<MODE, NG, 0, 3>), dim3(grid), dim3(kBlock), lds, s, p);
}

template <int MODE>
static void launch_distinct_ng(const KParams& p, int ng, int grid, size_t lds, hipStream_t s) {
  switch (ng) {
    case 1: launch_distinct_scan<MODE, 1>(p, grid, lds, s); break;
    case 2: launch_distinct_scan<MODE, 2>(p, grid, lds, s); break;
    case 3: launch_distinct_scan<MODE, 3>(p, grid, lds, s); break;
    default: launch_distinct_scan<MODE, 4>(p, grid, lds, s); break;
  }
}

void launch_scan_distinct(const KParams& p, int mode, int ng, int grid, size_t lds, hipStream_t s) {
  if (!p.out_dc || p.num_dc <= 0 || p.num_dc > kMaxHll || p.dc_row_words <= 0)
    fail(PH_ERR_INVALID_ARGUMENT, "DISTINCTCOUNT scan without a bitset table");
  switch (mode) {
    case MODE_AGG: launch_distinct_scan<MODE_AGG, 0>(p, grid, lds, s); break;
    case MODE_GROUP_LDS: launch_distinct_ng<MODE_GROUP_LDS>(p, ng, grid, lds, s); break;
    case MODE_GROUP_GLOBAL: launch_distinct_ng<MODE_GROUP_GLOBAL>(p, ng, grid, lds, s); break;
    default: fail(PH_ERR_UNSUPPORTED, "DISTINCTCOUNT in this plan mode");
  }
  PH_HIP_CHECK(hipGetLastError());
}

}  // namespace ph
