// regex_dict.hip -- k_regex_dict: the dictIds of a STRING dictionary whose value a REGEXP_LIKE pattern finds a match
// in, the dictionary-based evaluator of the reference (RegexpLikePredicateEvaluatorFactory.java:79-81:
// matcher.reset(dictionary.getStringValue(id)).find()) for every dictId at once.  The pattern is compiled on the host
// (regex_compile, regex_dfa.cpp) into a byte-level DFA, a RegexProgram of up to 16.3 KiB that is uploaded to query
// scratch and copied to LDS by every workgroup.
//
// The dictionary is the pinned buffer k_like_dict reads (Column::d_strings: `card` entries of `width` bytes, UTF-8,
// zero padded, and padded with zero entries to whole 256-entry tiles), and the tile staging is that kernel's, restated:
// a workgroup of T threads takes tiles of T entries, thread t loads the 16-byte chunks t, t + T, ... of the tile
// (coalesced dwordx4) into registers, the chunks are written to LDS row by row with the row stride padded to an odd
// number of dwords, and the next tile's chunks are loaded while this tile is walked.
//
// The walk is this kernel's own.  A DFA reads strictly forward with one byte of state, so a lane reads its row a dword
// at a time (rows are dword aligned by the stride) and peels the four bytes from the register: one LDS read of the row
// per four bytes, then per byte one read of the class map and one of the table.  The length scan reads the same dwords.
// The wave leaves the loop once every lane is at its value's end or in the (absorbing) accept state.  Bytes at or past
// `width` in a row's last dword were never written when rows are written bytewise; neither the length scan nor the
// walk looks at them.  Verdicts leave as k_like_dict's do: one __ballot word per wave stored by lane 0, one atomic of
// its popcount.
#include <string>

#include "ph_internal.h"

namespace ph {

namespace {

constexpr int kRegexTileBytes = 32768;  // LDS budget of a tile's rows; with the largest program under 49 KiB
constexpr int kRegexMaxWidth = 256;     // 16 chunks of 16 bytes per thread

struct LdsDwordRow {
  const uint32_t* p;
  __device__ uint32_t dword(int i) const { return p[i]; }
};

}  // namespace

// NL: 16-byte chunks a thread holds per tile (ceil(width / 16) rounded up to a compiled form)
template <int NL>
__global__ void __launch_bounds__(256) k_regex_dict(const uint8_t* __restrict__ dict, int32_t card, int32_t width,
                                                    int32_t stride, int32_t ntiles,
                                                    const uint4* __restrict__ prog, int32_t prog_chunks,
                                                    unsigned long long* __restrict__ bitmap,
                                                    unsigned long long* __restrict__ count) {
  extern __shared__ uint4 lds[];  // the program (prog_chunks of 16 bytes), then the tile
  const RegexHeader& hdr = *reinterpret_cast<const RegexHeader*>(lds);
  const uint8_t* next = reinterpret_cast<const uint8_t*>(lds) + sizeof(RegexHeader);
  uint8_t* tile = reinterpret_cast<uint8_t*>(lds + prog_chunks);
  const int T = (int)blockDim.x, t = (int)threadIdx.x;
  for (int i = t; i < prog_chunks; i += T) lds[i] = prog[i];

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
    __syncthreads();  // the previous tile's walks are done with the rows (and the program is written)
    stash();
    __syncthreads();
    const int nxt = tl + (int)gridDim.x;
    if (nxt < ntiles) load(nxt);  // in flight while this tile is walked
    const LdsDwordRow row{reinterpret_cast<const uint32_t*>(tile + (uint32_t)t * (uint32_t)stride)};
    const int64_t entry = (int64_t)tl * T + t;
    const int len = entry < card ? regex_row_len(row, width) : 0;
    const int dollar = regex_dollar_place(row, len);
    uint32_t s = (uint32_t)hdr.start;
    // wave-uniform trips: a lane past its end or already accepting feeds nothing
    for (int i = 0; __any(i < len && !regex_accepts(s, hdr)); i += 4)
      if (i < len) s = regex_feed_dword(s, row.dword(i >> 2), i, len, dollar, hdr, next);
    s = next[s * (uint32_t)hdr.nclasses + (uint32_t)hdr.mark];
    const bool m = entry < card && regex_accepts(s, hdr);
    const unsigned long long b = __ballot(m);
    if ((t & 63) == 0) {
      const int64_t word = entry >> 6;
      if (word < nwords) bitmap[word] = b;
      if (b) atomicAdd(count, (unsigned long long)__popcll(b));
    }
  }
}

void regex_tile_shape(int32_t width, int32_t* tile_entries, int32_t* stride_bytes) {
  const int32_t stride = 4 * (((width + 3) / 4) | 1);  // an odd number of dwords
  *stride_bytes = stride;
  *tile_entries = 0;
  if (width > kRegexMaxWidth) return;
  for (int32_t t = 256; t >= 64; t /= 2)
    if ((int64_t)t * stride <= kRegexTileBytes) {
      *tile_entries = t;
      return;
    }
}

void launch_regex_dict(const uint8_t* dict, int32_t card, int32_t width, const uint8_t* prog, uint32_t prog_bytes,
                       unsigned long long* bitmap, unsigned long long* count, int num_cus, hipStream_t s) {
  if (card <= 0) return;
  int32_t T = 0, stride = 0;
  regex_tile_shape(width, &T, &stride);
  if (!T)
    fail(PH_ERR_UNSUPPORTED, "REGEXP_LIKE: dictionary entries of " + std::to_string(width) +
                                 " bytes are wider than the kernel's LDS tile");
  const int ntiles = (int)(((int64_t)card + T - 1) / T);
  const int grid = std::max(1, std::min(ntiles, 4 * std::max(1, num_cus)));
  const int prog_chunks = (int)(prog_bytes / 16);
  const size_t lds = (size_t)prog_bytes + ((size_t)T * stride + 15) / 16 * 16;  // under 64 KiB: no launch attribute
  const int nl = (width + 15) / 16;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3((unsigned)T), lds, s, dict, card, width, stride, ntiles,
                       reinterpret_cast<const uint4*>(prog), prog_chunks, bitmap, count);
  };
  if (nl <= 2) go(k_regex_dict<2>);
  else if (nl <= 8) go(k_regex_dict<8>);
  else go(k_regex_dict<16>);
  PH_HIP_CHECK(hipGetLastError());
}

}  // namespace ph
