// scan_hll_sketch.hip -- DISTINCTCOUNTHLL served from a star-tree's distinctCountHLL__<col> pair column.
//
// A star-tree record holds a whole HyperLogLog (DistinctCountHLLValueAggregator: the pre-aggregated sketch of the raw
// documents under the record), not a value to hash: aggregating it is HyperLogLog.addAll, a register-wise max of
// 2^log2m registers (DistinctCountHLLValueAggregator.java:89-97,116).  The view pins the records' RegisterSet words
// (six 5-bit registers per 32-bit word, register i in word i / 6 at shift 5 * (i % 6)) as one block per pair column.
//
//   k_scan<.., LATE = 2>   the generic scan; for a sketch slot a matched record appends (launch-wide document << 32 |
//                          row base in out_hll) to the launch's match list instead of looking a table entry up
//   k_hll_sketch_merge     right after it on the same stream, grid-strided over the device-side entry count (no host
//                          round trip): one wave per entry, the lanes read the record's words coalesced (ceil(words /
//                          64) passes, the last one partial), unpack six registers each, skip zeros and registers at
//                          index >= m (the last word's tail), and atomicMax the rest into out_hll -- after a plain read:
//                          a register already that high costs no atomic (most of them once a row has warmed up)
//
// Only sketch queries instantiate LATE = 2, over the general value-column variant (REC64 = 0).
#include <algorithm>

#include "scan_kernel.h"

namespace ph {

__global__ void __launch_bounds__(kBlock) k_hll_sketch_merge(const KParams p) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * kBlock + threadIdx.x) >> 6));
  const uint32_t nwaves = gridDim.x * kWaves;
  const uint32_t n = min(gld(p.sk_count), p.sk_cap);
  const uint32_t m = 1u << p.log2m;
  SegPtr segs = (SegPtr)p.segs;
  for (uint32_t e = wave; e < n; e += nwaves) {
    const unsigned long long ent = gld(p.sk_list + e);
    const uint32_t base = (uint32_t)ent, gdoc = (uint32_t)(ent >> 32);
    // the entry's segment: the last one whose first document is <= gdoc (an empty segment shares its successor's)
    int lo = 0, hi = p.num_segs - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (segs[mid].sk_doc_base <= gdoc) lo = mid;
      else hi = mid - 1;
    }
    SegPtr S = segs + lo;
    const uint32_t h = (base >> p.log2m) % (uint32_t)p.num_hll;
    ColRef col = S->cols[p.hll_slot[h]];
    const uint32_t doc = gdoc - S->sk_doc_base;
    const int32_t words = col.sketch_words;
    if (!col.sketch || doc >= (uint32_t)S->num_docs) continue;
    const uint32_t* rec = col.sketch + (size_t)doc * (size_t)words;
    uint32_t* row = p.out_hll + base;
    for (int32_t w = lane; w < words; w += 64) {
      uint32_t x = gld(rec + w);
#pragma unroll
      for (uint32_t k = 0; k < 6; ++k) {
        const uint32_t r = x & 31u, i = 6u * (uint32_t)w + k;
        x >>= 5;
        if (r && i < m && __hip_atomic_load(row + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < r) atomicMax(row + i, r);
      }
    }
  }
}

template <int MODE, int NG>
static void launch_sketch_scan(const KParams& p, int grid, size_t lds, hipStream_t s) {
  allow_lds(k_scan<MODE, NG, 0, 2>, lds);
  hipLaunchKernelGGL((k_scan<MODE, NG, 0, 2>), dim3(grid), dim3(kBlock), lds, s, p);
}

template <int MODE>
static void launch_sketch_ng(const KParams& p, int ng, int grid, size_t lds, hipStream_t s) {
  switch (ng) {
    case 1: launch_sketch_scan<MODE, 1>(p, grid, lds, s); break;
    case 2: launch_sketch_scan<MODE, 2>(p, grid, lds, s); break;
    case 3: launch_sketch_scan<MODE, 3>(p, grid, lds, s); break;
    default: launch_sketch_scan<MODE, 4>(p, grid, lds, s); break;
  }
}

void launch_scan_sketch(const KParams& p, int mode, int ng, int grid, size_t lds, hipStream_t s) {
  if (!p.sk_list || !p.sk_count || !p.out_hll || p.num_segs <= 0) fail(PH_ERR_INVALID_ARGUMENT, "sketch scan without a match list");
  switch (mode) {
    case MODE_AGG: launch_sketch_scan<MODE_AGG, 0>(p, grid, lds, s); break;
    case MODE_GROUP_LDS: launch_sketch_ng<MODE_GROUP_LDS>(p, ng, grid, lds, s); break;
    case MODE_GROUP_GLOBAL: launch_sketch_ng<MODE_GROUP_GLOBAL>(p, ng, grid, lds, s); break;
    case MODE_GROUP_HASH: launch_sketch_ng<MODE_GROUP_HASH>(p, ng, grid, lds, s); break;
    default: fail(PH_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL over a sketch column in this plan mode");
  }
  PH_HIP_CHECK(hipGetLastError());
  // one wave per entry; the entry count stays on the device, so the grid is sized by the list's capacity
  const uint32_t blocks = std::max<uint32_t>(1u, std::min<uint32_t>((p.sk_cap + kWaves - 1) / kWaves, 2048u));
  hipLaunchKernelGGL(k_hll_sketch_merge, dim3(blocks), dim3(kBlock), 0, s, p);
  PH_HIP_CHECK(hipGetLastError());
  PH_HIP_CHECK(hipMemsetAsync(p.sk_count, 0, sizeof(uint32_t), s));  // the next launch of the call appends from 0
}

}  // namespace ph
