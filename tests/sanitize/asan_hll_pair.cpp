// asan_hll_pair.cpp -- CPU sanitizer harness of the star-tree distinctCountHLL pair parser (rawfwd.cpp:
// var_byte_forward_index_read + hll_pair_column_parse, what ph_star_tree_hll_pair_check and ph_segment_add_star_tree
// run on untrusted bytes), built with -fsanitize=address,undefined.  Test infrastructure only
// (tests/test_startree_hll_cpu.py).
//
// It writes valid pair columns itself (writer versions 2 and 3, PASS_THROUGH, log2m 4 / 8 / 12, a partial last chunk)
// and parses: every prefix of each (truncation at every byte), a value one word short, two records of different
// log2m, a chunk offset past the buffer, a value offset past its chunk, more docs than the file holds, extreme values
// in every header field, and seeded bit flips.  Then every `<file> <numDocs>` pair of the command line (the buffers
// the Python test mutates).  Each buffer is copied to an exactly-sized heap block first, so a read past its end is an
// AddressSanitizer report.  Every parse must succeed or throw ph::Error; a report aborts (-fno-sanitize-recover=all).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include <string>
#include <vector>

#include "ph_internal.h"

namespace ph {
[[noreturn]] void fail(int code, const std::string& msg) { throw Error{code, msg}; }
}  // namespace ph

namespace {

typedef std::vector<uint8_t> Bytes;

void put32(Bytes& b, uint32_t v) {
  for (int k = 3; k >= 0; --k) b.push_back((uint8_t)(v >> (8 * k)));
}
void put64(Bytes& b, uint64_t v) {
  put32(b, (uint32_t)(v >> 32));
  put32(b, (uint32_t)v);
}
void set32(Bytes& b, size_t at, uint32_t v) {
  for (int k = 0; k < 4; ++k) b[at + k] = (uint8_t)(v >> (8 * (3 - k)));
}

Bytes hll_value(int log2m, std::mt19937& rng, int short_words = 0) {
  const uint32_t words = (1u << log2m) / 6 + 1 - (uint32_t)short_words;
  Bytes v;
  put32(v, (uint32_t)log2m);
  put32(v, 4 * ((1u << log2m) / 6 + 1));
  for (uint32_t w = 0; w < words; ++w) put32(v, (uint32_t)rng() & 0x3fffffffu);
  return v;
}

Bytes write_var_byte(const std::vector<Bytes>& vals, int version, int per_chunk) {
  const int n = (int)vals.size(), nchunks = (n + per_chunk - 1) / per_chunk, osz = version == 2 ? 4 : 8;
  size_t longest = 0;
  for (auto& v : vals) longest = std::max(longest, v.size());
  std::vector<Bytes> chunks;
  for (int c = 0; c < nchunks; ++c) {
    Bytes head, body;
    uint32_t at = 4u * (uint32_t)per_chunk;
    for (int r = 0; r < per_chunk; ++r) {
      const int d = c * per_chunk + r;
      put32(head, d < n ? at : 0u);
      if (d < n) {
        body.insert(body.end(), vals[d].begin(), vals[d].end());
        at += (uint32_t)vals[d].size();
      }
    }
    head.insert(head.end(), body.begin(), body.end());
    chunks.push_back(head);
  }
  Bytes out;
  for (uint32_t h : {(uint32_t)version, (uint32_t)nchunks, (uint32_t)per_chunk, (uint32_t)longest, (uint32_t)n, 0u, 28u})
    put32(out, h);
  uint64_t pos = 28 + (uint64_t)nchunks * osz;
  for (auto& c : chunks) {
    if (osz == 4) put32(out, (uint32_t)pos);
    else put64(out, pos);
    pos += c.size();
  }
  for (auto& c : chunks) out.insert(out.end(), c.begin(), c.end());
  return out;
}

long g_ok = 0, g_rejected = 0;

// 0 = parsed, else the error code
int parse(const Bytes& b, int64_t num_docs, int32_t* log2m = nullptr) {
  uint8_t* exact = static_cast<uint8_t*>(malloc(b.size() ? b.size() : 1));  // (exact size: a redzone right behind)
  if (!b.empty()) memcpy(exact, b.data(), b.size());
  int code = 0;
  try {
    int32_t lm = 0;
    std::vector<uint32_t> words;
    ph::hll_pair_column_parse(exact, b.size(), num_docs, "distinctCountHLL__c", &lm, &words);
    if (log2m) *log2m = lm;
    ++g_ok;
  } catch (const ph::Error& e) {
    code = e.code;
    ++g_rejected;
  }
  free(exact);
  return code;
}

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "asan_hll_pair: %s (line %d)\n", #cond, __LINE__); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

}  // namespace

int main(int argc, char** argv) {
  std::mt19937 rng(20240611);
  for (int version : {2, 3})
    for (int log2m : {4, 8, 12}) {
      const int n = log2m == 12 ? 7 : 23, per_chunk = log2m == 12 ? 3 : 10;
      std::vector<Bytes> vals;
      for (int i = 0; i < n; ++i) vals.push_back(hll_value(log2m, rng));
      const Bytes good = write_var_byte(vals, version, per_chunk);
      int32_t lm = 0;
      EXPECT(parse(good, n, &lm) == 0 && lm == log2m);
      EXPECT(parse(good, n - 1, &lm) == 0 && lm == log2m);  // fewer docs than the file holds is a prefix
      EXPECT(parse(good, n + 1) == PH_ERR_INVALID_ARGUMENT);
      EXPECT(parse(good, 0) == PH_ERR_INVALID_ARGUMENT);
      for (size_t cut = 0; cut < good.size(); ++cut)
        EXPECT(parse(Bytes(good.begin(), good.begin() + (long)cut), n) == PH_ERR_INVALID_ARGUMENT);
      {  // a value one word short
        std::vector<Bytes> v2 = vals;
        v2[n / 2] = hll_value(log2m, rng, 1);
        EXPECT(parse(write_var_byte(v2, version, per_chunk), n) == PH_ERR_INVALID_ARGUMENT);
      }
      {  // two records of different log2m
        std::vector<Bytes> v2 = vals;
        v2[n - 1] = hll_value(log2m == 4 ? 5 : log2m - 1, rng);
        EXPECT(parse(write_var_byte(v2, version, per_chunk), n) == PH_ERR_INVALID_ARGUMENT);
      }
      const size_t osz = version == 2 ? 4 : 8;
      {  // a chunk offset past the buffer
        Bytes b = good;
        set32(b, 28 + osz - 4, (uint32_t)good.size() + 64);
        EXPECT(parse(b, n) == PH_ERR_INVALID_ARGUMENT);
      }
      {  // a value offset past its chunk
        Bytes b = good;
        const size_t nchunks = (size_t)((n + per_chunk - 1) / per_chunk);
        set32(b, 28 + nchunks * osz + 4, 0x7fffff00u);
        EXPECT(parse(b, n) == PH_ERR_INVALID_ARGUMENT);
      }
      for (size_t field = 0; field < 7; ++field)  // extreme header fields: an error or (totalDocs) still a valid parse
        for (uint32_t x : {0u, 1u, 0x7fffffffu, 0x80000000u, 0xffffffffu}) {
          Bytes b = good;
          set32(b, 4 * field, x);
          (void)parse(b, n);
        }
      for (int it = 0; it < 400; ++it) {  // seeded bit flips (any outcome but a sanitizer report)
        Bytes b = good;
        const int flips = 1 + (int)(rng() % 3);
        for (int f = 0; f < flips; ++f) b[rng() % b.size()] ^= (uint8_t)(1u << (rng() % 8));
        (void)parse(b, n);
      }
    }
  for (int i = 1; i + 1 < argc; i += 2) {
    std::ifstream in(argv[i], std::ios::binary);
    const Bytes b((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const int code = parse(b, atol(argv[i + 1]));
    printf("%s %d\n", argv[i], code);
  }
  printf("parsed %ld, rejected %ld: no sanitizer report\n", g_ok, g_rejected);
  return 0;
}
