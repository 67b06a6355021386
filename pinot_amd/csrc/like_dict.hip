// like_dict.hip -- k_like_dict: the dictIds of a STRING dictionary whose value a LIKE pattern matches, the
// dictionary-based evaluator of the reference's REGEXP_LIKE (DictionaryBasedRegexpLikePredicateEvaluator.applySV,
// RegexpLikePredicateEvaluatorFactory.java:79-81: matcher.reset(dictionary.getStringValue(id)).find()), for every
// dictId at once.  The pattern is compiled on the host (like_compile: the reference's likeToRegexpLike restated as a
// list of segments, like_match.h) into a LikeProgram that travels in the kernel arguments and is copied to LDS.
//
// The dictionary is the pinned buffer as the segment stores it: `card` entries of `width` bytes, UTF-8, zero padded
// (Column::d_strings, padded with zero entries to whole 256-entry tiles).  A workgroup of T threads takes tiles of T
// entries (T = 256, or 128 / 64 when the rows of 256 entries pass the LDS budget), a wave 64 of them:
//   1. a tile is T * width contiguous bytes: thread t loads its 16-byte chunks t, t + T, ... (coalesced dwordx4) into
//      registers;
//   2. the chunks are written into LDS row by row with the row stride padded to an odd number of dwords, so the 64
//      lanes of a wave, each walking its own row, start on 64 different banks;
//   3. the NEXT tile's chunks are loaded into the registers (they stay in flight during the match);
//   4. every lane finds its entry's length (the first zero byte) and runs like_match on its row out of LDS;
//   5. the wave's verdicts are one __ballot: lane 0 stores that 64-bit word of the dictId bitmap (a plain vector
//      store; every word of the bitmap is written by exactly one wave) and adds its popcount to the match counter
//      with one atomic.
// Registers, not a second LDS buffer, hold the tile in flight, so the LDS tile is single: 32 KiB at most.
#include <string>

#include "ph_internal.h"

namespace ph {

namespace {

constexpr int kLikeTileBytes = 32768;  // LDS budget of a tile's rows
constexpr int kLikeMaxWidth = 256;     // 16 chunks of 16 bytes per thread: the widest form that needs no scratch

struct LdsRow {
  const uint8_t* p;
  __device__ uint32_t operator[](int i) const { return p[i]; }
};

}  // namespace

// NL: 16-byte chunks a thread holds per tile (ceil(width / 16) rounded up to a compiled form)
template <int NL>
__global__ void __launch_bounds__(256) k_like_dict(const uint8_t* __restrict__ dict, int32_t card, int32_t width,
                                                   int32_t stride, int32_t ntiles, LikeProgram prog,
                                                   unsigned long long* __restrict__ bitmap,
                                                   unsigned long long* __restrict__ count) {
  extern __shared__ uint4 lds_tile[];
  __shared__ LikeProgram sp;
  uint8_t* tile = reinterpret_cast<uint8_t*>(lds_tile);
  const int T = (int)blockDim.x, t = (int)threadIdx.x;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&prog);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&sp);
    for (int i = t; i < (int)(sizeof(LikeProgram) / 4); i += T) dst[i] = src[i];
  }
  const uint32_t tile_bytes = (uint32_t)T * (uint32_t)width;  // a multiple of 16: T is a multiple of 64
  const uint32_t chunks = tile_bytes / 16;
  const bool dword_rows = (width & 3) == 0;
  const int64_t nwords = ((int64_t)card + 63) / 64;

  uint4 r[NL];
  auto load = [&](int tl) {
    const uint4* g = reinterpret_cast<const uint4*>(dict + (size_t)tl * tile_bytes);
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const uint32_t c = (uint32_t)t + (uint32_t)j * (uint32_t)T;
      r[j] = c < chunks ? g[c] : make_uint4(0, 0, 0, 0);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const uint32_t c = (uint32_t)t + (uint32_t)j * (uint32_t)T;
      if (c >= chunks) continue;
      const uint32_t w[4] = {r[j].x, r[j].y, r[j].z, r[j].w};
      uint32_t row = 16u * c / (uint32_t)width;
      uint32_t col = 16u * c - row * (uint32_t)width;
      if (dword_rows) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          *reinterpret_cast<uint32_t*>(tile + row * (uint32_t)stride + col) = w[q];
          col += 4;
          if (col >= (uint32_t)width) { col = 0; ++row; }
        }
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          tile[row * (uint32_t)stride + col] = (uint8_t)(w[q >> 2] >> (8 * (q & 3)));
          if (++col == (uint32_t)width) { col = 0; ++row; }
        }
      }
    }
  };

  int tl = (int)blockIdx.x;  // the trip count is uniform over the workgroup
  if (tl < ntiles) load(tl);
  for (; tl < ntiles; tl += (int)gridDim.x) {
    __syncthreads();  // the previous tile's matches are done with the rows (and sp is written)
    stash();
    __syncthreads();
    const int next = tl + (int)gridDim.x;
    if (next < ntiles) load(next);  // in flight while this tile matches
    const LdsRow row{tile + (uint32_t)t * (uint32_t)stride};
    int len = 0;
    while (len < width && row[len] != 0) ++len;
    const int64_t entry = (int64_t)tl * T + t;
    const bool m = entry < card && like_match(row, len, sp);
    const unsigned long long b = __ballot(m);
    if ((t & 63) == 0) {
      const int64_t word = entry >> 6;
      if (word < nwords) bitmap[word] = b;
      if (b) atomicAdd(count, (unsigned long long)__popcll(b));
    }
  }
}

// RegexpPatternConverterUtils.likeToRegexpLike (:43-131) restated as the segments of the regex it would emit.  The
// converter keeps a backslash it has just copied "pending": the next character decides whether it escapes a wildcard
// (\_ and \% are literals) or is itself escaped into a literal backslash.
LikeProgram like_compile(const std::string& pat) {
  LikeProgram P{};
  P.anchor_start = P.anchor_end = 1;
  size_t start = 0, end = pat.size();
  if (pat.empty()) {  // "^$"
    P.nseg = 1;
    return P;
  }
  // runs of `%` at either end drop that side's anchor; the trailing run is cut without a look at an escape before it
  if (pat.front() == '%') {
    start = pat.find_first_not_of('%');
    if (start == std::string::npos) {  // "": matches everything
      P.nseg = 0;
      return P;
    }
    P.anchor_start = 0;
  }
  if (pat.size() > 1 && pat.back() == '%') {
    end = pat.find_last_not_of('%') + 1;
    P.anchor_end = 0;
  }
  int nel = 0, seg = 0, seg_len = 0;
  bool open = false;  // a segment has elements
  auto element = [&](uint8_t byte, bool wild) {
    if (!open) {
      if (seg >= kLikeMaxSegs)
        fail(PH_ERR_UNSUPPORTED, "LIKE pattern has more than " + std::to_string(kLikeMaxSegs) +
                                     " runs between % wildcards");
      P.off[seg] = (uint16_t)nel;
      open = true;
      seg_len = 0;
    }
    if (nel >= kLikeMaxBytes)
      fail(PH_ERR_UNSUPPORTED, "LIKE pattern is longer than " + std::to_string(kLikeMaxBytes) + " bytes");
    if (seg_len >= kLikeSegElems)
      fail(PH_ERR_UNSUPPORTED, "LIKE pattern has a run of more than " + std::to_string(kLikeSegElems) +
                                   " bytes between % wildcards");
    if (byte == '\n' || byte == '\r')
      fail(PH_ERR_UNSUPPORTED, "LIKE pattern holds a line terminator");
    P.elems[nel++] = wild ? 0 : byte;
    if (wild) P.wild[seg] |= 1ull << seg_len;
    P.len[seg] = (uint16_t)++seg_len;
  };
  auto close = [&]() {
    if (open) ++seg;
    open = false;
  };
  static const char kMeta[] = "^$.{}[]()*+?|<>-&/";  // REGEXP_METACHARACTERS
  bool pending = false;  // an unresolved backslash
  for (size_t i = start; i < end; ++i) {
    const uint8_t c = (uint8_t)pat[i];
    if (c == '_') {
      element('_', !pending);
      pending = false;
    } else if (c == '%') {
      if (pending) element('%', false);
      else close();
      pending = false;
    } else if (c == '\\') {
      if (pending) element('\\', false);  // the earlier one, escaped by this one's turn
      pending = true;
    } else {
      if (pending) {
        // the converter emits one backslash here, which escapes the pending one and leaves a metacharacter bare
        if (c < 0x80 && strchr(kMeta, (int)c))
          fail(PH_ERR_UNSUPPORTED, "LIKE pattern has a backslash before the regex metacharacter " + std::string(1, (char)c));
        element('\\', false);
      }
      element(c, false);
      pending = false;
    }
  }
  if (pending) element('\\', false);  // a trailing backslash is a literal
  close();
  // U+0085, U+2028, U+2029 as literals: like \n and \r, no `.` of the emitted regex could sit beside them in a line
  for (int i = 0; i + 1 < nel; ++i) {
    const uint8_t* e = P.elems + i;
    if ((e[0] == 0xC2 && e[1] == 0x85) || (i + 2 < nel && e[0] == 0xE2 && e[1] == 0x80 && (e[2] | 1) == 0xA9))
      fail(PH_ERR_UNSUPPORTED, "LIKE pattern holds a line terminator");
  }
  P.nseg = seg;
  return P;
}

void like_tile_shape(int32_t width, int32_t* tile_entries, int32_t* stride_bytes) {
  const int32_t stride = 4 * (((width + 3) / 4) | 1);  // an odd number of dwords
  *stride_bytes = stride;
  *tile_entries = 0;
  if (width > kLikeMaxWidth) return;
  for (int32_t t = 256; t >= 64; t /= 2)
    if ((int64_t)t * stride <= kLikeTileBytes) {
      *tile_entries = t;
      return;
    }
}

// the dictionary buffer k_like_dict reads: whole 256-entry tiles, so no tile's loads leave it
size_t like_dict_alloc_bytes(int64_t card, int32_t width) {
  return (size_t)((card + 255) / 256 * 256) * (size_t)width + 16;
}

void launch_like_dict(const uint8_t* dict, int32_t card, int32_t width, const LikeProgram& prog,
                      unsigned long long* bitmap, unsigned long long* count, int num_cus, hipStream_t s) {
  if (card <= 0) return;
  int32_t T = 0, stride = 0;
  like_tile_shape(width, &T, &stride);
  if (!T)
    fail(PH_ERR_UNSUPPORTED, "LIKE: dictionary entries of " + std::to_string(width) +
                                 " bytes are wider than the kernel's LDS tile");
  const int ntiles = (int)(((int64_t)card + T - 1) / T);
  const int grid = std::max(1, std::min(ntiles, 4 * std::max(1, num_cus)));
  const size_t lds = ((size_t)T * stride + 15) / 16 * 16;
  const int nl = (width + 15) / 16;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3((unsigned)T), lds, s, dict, card, width, stride, ntiles, prog,
                       bitmap, count);
  };
  if (nl <= 2) go(k_like_dict<2>);
  else if (nl <= 8) go(k_like_dict<8>);
  else go(k_like_dict<16>);
  PH_HIP_CHECK(hipGetLastError());
}

}  // namespace ph
