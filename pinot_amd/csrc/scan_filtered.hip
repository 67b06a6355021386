// scan_filtered.hip -- filtered aggregations (agg(...) FILTER(WHERE ...)) in one pass over the wide columns.
//
// The reference runs one filter -> projection -> aggregation pipeline per distinct FILTER clause plus one for the
// unfiltered functions (AggregationFunctionUtils.buildFilteredAggregateProjectOperators,
// AggregationFunctionUtils.java:191-267; FilteredAggregationOperator.java:66-94, FilteredGroupByOperator.java:107-190):
// K + 1 passes over the group-by and value columns.  Here a pipeline is one bit per doc: stage 1 (filtered.cpp) leaves
// a doc bitmap per filter in HBM, and k_scan_filtered reads the group-by and value streams once.
//
// Per 64-doc word a wave loads every pipeline's mask word -- (a & b) of two optional bitmaps, main and sub-filter; a
// missing bitmap matches all -- and skips the word when their union is zero.  Lane l owns doc 64 w + l: a lane of the
// union decodes its group key and the value terms once, and feeds aggregation slot s only where the bit of slot s's
// pipeline is set.
//   MODE_AGG           per-lane accumulators, wave reductions, the workgroup's waves combined in LDS, then one atomic
//                      per workgroup per slot
//   MODE_GROUP_LDS     per-workgroup dense tables in LDS ([pipelines + slots][groups] 8-byte cells), flushed to the HBM
//                      tables at the end (identity cells skipped)
//   MODE_GROUP_GLOBAL  device atomics straight into the HBM tables
// The per-pipeline doc counts per group (FParams::pcount) are COUNT(*)'s result, the presence test of a result row
// (a group is a row when any pipeline saw a doc of it) and the test for an empty cell's default.  The docs each
// pipeline matched per segment (FParams::seg_count: wave-uniform popcounts, one atomic per chunk per pipeline) give the
// statistics and, without a group-by, COUNT(*).
#include <algorithm>

#include "scan_kernel.h"

namespace ph {

typedef const PH_CONST FSegment* FSegPtr;

__device__ __forceinline__ unsigned long long f_mask_word(FSegPtr S, int p, int32_t w, unsigned long long tail) {
  if ((S->empty >> p) & 1u) return 0ull;
  const unsigned long long* a = S->ma[p];
  const unsigned long long* b = S->mb[p];
  unsigned long long m = tail;
  if (a) m &= gld(a + w);
  if (b) m &= gld(b + w);
  return m;
}

__device__ __forceinline__ long long f_identity(int op) {
  return (op == FOP_MIN_I || op == FOP_MIN_F) ? INT64_MAX : ((op == FOP_MAX_I || op == FOP_MAX_F) ? INT64_MIN : 0ll);
}

// the 8-byte cell value slot op `op` adds / compares for a doc whose term is `bits` (an int64, or a double's bits)
__device__ __forceinline__ long long f_operand(int op, long long bits) {
  switch (op) {
    case FOP_SUM_I2F: return __double_as_longlong((double)bits);
    case FOP_MIN_F: return min_order_key(double_order_key(__longlong_as_double(bits)), __longlong_as_double(bits));
    case FOP_MAX_F: return max_order_key(double_order_key(__longlong_as_double(bits)), __longlong_as_double(bits));
    default: return bits;
  }
}

__device__ __forceinline__ long long f_combine(int op, long long a, long long b) {
  switch (op) {
    case FOP_SUM_I: return (long long)((unsigned long long)a + (unsigned long long)b);
    case FOP_SUM_F:
    case FOP_SUM_I2F: return __double_as_longlong(__longlong_as_double(a) + __longlong_as_double(b));
    case FOP_MIN_I:
    case FOP_MIN_F: return b < a ? b : a;
    default: return b > a ? b : a;
  }
}

__device__ __forceinline__ void f_atomic(int op, long long* cell, long long v) {
  switch (op) {
    case FOP_SUM_I: atomicAdd(reinterpret_cast<unsigned long long*>(cell), (unsigned long long)v); break;
    case FOP_SUM_F:
    case FOP_SUM_I2F: atomicAdd(reinterpret_cast<double*>(cell), __longlong_as_double(v)); break;
    case FOP_MIN_I:
    case FOP_MIN_F: atomicMin(cell, v); break;
    default: atomicMax(cell, v); break;
  }
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) k_scan_filtered(const FParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char f_lds[];
  long long* lds = reinterpret_cast<long long*>(f_lds);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int np = p.num_pipes, ns = p.num_slots;
  const int64_t G = p.num_groups;

  if (MODE == MODE_GROUP_LDS) {
    for (int64_t i = threadIdx.x; i < (int64_t)(np + ns) * G; i += kBlock) {
      const int t = (int)(i / G);
      lds[i] = t < np ? 0ll : f_identity(p.slot_op[t - np]);
    }
    __syncthreads();
  }

  long long acc[kFMaxSlots];
#pragma unroll
  for (int s = 0; s < kFMaxSlots; ++s) acc[s] = s < ns ? f_identity(p.slot_op[s]) : 0ll;

  for (int c = p.chunk_begin + (int)blockIdx.x; c < p.chunk_end; c += (int)gridDim.x) {
    const PH_CONST Chunk* ck = (const PH_CONST Chunk*)p.chunks + c;  // C-style cast = addrspacecast
    const int32_t seg = ck->seg, wb = ck->word_begin, we = ck->word_end;
    FSegPtr S = (FSegPtr)p.segs + seg;
    const int32_t nd = S->num_docs;
    unsigned long long pc[kFMaxPipes];  // wave-uniform: this wave's docs of the chunk per pipeline
#pragma unroll
    for (int q = 0; q < kFMaxPipes; ++q) pc[q] = 0ull;
    for (int32_t w = wb + wave; w < we; w += kWaves) {
      const int32_t left = nd - w * 64;
      if (left <= 0) break;
      const unsigned long long tail = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
      unsigned long long uni = 0ull;
      unsigned long long mw[kFMaxPipes];  // the word's mask per pipeline: wave-uniform, loaded once
#pragma unroll
      for (int q = 0; q < kFMaxPipes; ++q) {
        mw[q] = q < np ? f_mask_word(S, q, w, tail) : 0ull;
        uni |= mw[q];
        pc[q] += (unsigned long long)__popcll(mw[q]);
      }
      if (uni == 0ull) continue;
      if (!((uni >> lane) & 1ull)) continue;
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
#pragma unroll
        for (int q = 0; q < kFMaxPipes; ++q) {
          if ((mw[q] >> lane) & 1ull) {
            if (MODE == MODE_GROUP_LDS) atomicAdd(reinterpret_cast<unsigned long long*>(lds) + (int64_t)q * G + key, 1ull);
            else atomicAdd(p.pcount + (int64_t)q * G + key, 1ull);
          }
        }
      }
      long long val[kFMaxVals];
#pragma unroll
      for (int v = 0; v < kFMaxVals; ++v) {
        val[v] = 0;
        if (v < p.num_vals) {
          const uint32_t id = unpack_bits(S->vfwd[v], S->vbits[v], doc);
          val[v] = gld(reinterpret_cast<const long long*>(S->vtable[v]) + id);
        }
      }
#pragma unroll
      for (int s = 0; s < kFMaxSlots; ++s) {
        if (s < ns) {
          const int op = p.slot_op[s];
          const int sp = p.slot_pipe[s];
          unsigned long long pm = mw[0];
#pragma unroll
          for (int q = 1; q < kFMaxPipes; ++q) pm = sp == q ? mw[q] : pm;
          if ((pm >> lane) & 1ull) {
            const int vi = p.slot_val[s];
            long long bits = val[0];
#pragma unroll
            for (int v = 1; v < kFMaxVals; ++v) bits = vi == v ? val[v] : bits;
            const long long x = f_operand(op, bits);
            if (MODE == MODE_AGG) acc[s] = f_combine(op, acc[s], x);
            else if (MODE == MODE_GROUP_LDS) f_atomic(op, lds + (int64_t)(np + s) * G + key, x);
            else f_atomic(op, p.slot_out[s] + key, x);
          }
        }
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < kFMaxPipes; ++q)
        if (q < np && pc[q]) atomicAdd(p.seg_count + (int64_t)seg * kFMaxPipes + q, pc[q]);
    }
  }

  if (MODE == MODE_AGG) {
    // wave reductions, the workgroup's waves combined in LDS, one atomic per workgroup per slot
#pragma unroll
    for (int s = 0; s < kFMaxSlots; ++s) {
      if (s < ns) {
        const int op = p.slot_op[s];
        long long v = acc[s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = f_combine(op, v, (long long)__shfl_xor(v, o, 64));
        if (lane == 0) lds[wave * kFMaxSlots + s] = v;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < ns) {
      const int s = (int)threadIdx.x;
      const int op = p.slot_op[s];
      long long v = lds[s];
      for (int k = 1; k < kWaves; ++k) v = f_combine(op, v, lds[k * kFMaxSlots + s]);
      if (v != f_identity(op)) f_atomic(op, p.slot_out[s], v);
    }
  } else if (MODE == MODE_GROUP_LDS) {
    __syncthreads();
    for (int64_t i = threadIdx.x; i < (int64_t)(np + ns) * G; i += kBlock) {
      const int t = (int)(i / G);
      const int64_t g = i - (int64_t)t * G;
      const long long v = lds[i];
      if (t < np) {
        if (v) atomicAdd(p.pcount + (int64_t)t * G + g, (unsigned long long)v);
      } else {
        const int op = p.slot_op[t - np];
        // (a double SUM cell still at +0.0 adds nothing to a table that starts at +0.0)
        if (v != f_identity(op)) f_atomic(op, p.slot_out[t - np] + g, v);
      }
    }
  }
}

size_t filtered_lds_bytes(const FParams& p, int mode) {
  if (mode == MODE_AGG) return (size_t)kWaves * kFMaxSlots * 8;
  if (mode == MODE_GROUP_LDS) return (size_t)(p.num_pipes + p.num_slots) * (size_t)p.num_groups * 8;
  return 0;
}

void launch_scan_filtered(const FParams& p, int mode, int grid, hipStream_t s) {
  if (!p.segs || !p.chunks || !p.seg_count || p.num_pipes <= 0 || p.num_pipes > kFMaxPipes || p.num_slots < 0 ||
      p.num_slots > kFMaxSlots || p.num_vals < 0 || p.num_vals > kFMaxVals || p.num_group_cols < 0 ||
      p.num_group_cols > kMaxGroupCols || p.num_groups <= 0 || (mode != MODE_AGG && !p.pcount))
    fail(PH_ERR_INVALID_ARGUMENT, "filtered scan with bad parameters");
  for (int i = 0; i < p.num_slots; ++i)
    if (!p.slot_out[i] || p.slot_pipe[i] < 0 || p.slot_pipe[i] >= p.num_pipes || p.slot_val[i] < 0 ||
        p.slot_val[i] >= p.num_vals || p.slot_op[i] < FOP_SUM_I || p.slot_op[i] > FOP_MAX_F)
      fail(PH_ERR_INVALID_ARGUMENT, "filtered scan with a bad slot");
  const size_t lds = filtered_lds_bytes(p, mode);
  if (lds > 160 * 1024) fail(PH_ERR_INVALID_ARGUMENT, "filtered scan tables exceed the LDS of one CU");
  switch (mode) {
    case MODE_AGG:
      hipLaunchKernelGGL(k_scan_filtered<MODE_AGG>, dim3(grid), dim3(kBlock), lds, s, p);
      break;
    case MODE_GROUP_LDS:
      allow_lds(k_scan_filtered<MODE_GROUP_LDS>, lds);
      hipLaunchKernelGGL(k_scan_filtered<MODE_GROUP_LDS>, dim3(grid), dim3(kBlock), lds, s, p);
      break;
    case MODE_GROUP_GLOBAL:
      hipLaunchKernelGGL(k_scan_filtered<MODE_GROUP_GLOBAL>, dim3(grid), dim3(kBlock), lds, s, p);
      break;
    default: fail(PH_ERR_UNSUPPORTED, "filtered aggregations in this plan mode");
  }
  PH_HIP_CHECK(hipGetLastError());
}

}  // namespace ph
