// regex_dfa.h -- the compiled form of a REGEXP_LIKE pattern and its walker over one UTF-8 value, as k_regex_dict runs it
// per lane out of LDS (regex_dict.hip).  The compiler is regex_dfa.cpp.
//
// The reference evaluates REGEXP_LIKE with java.util.regex's Matcher.find() on every dictionary value
// (RegexpLikePredicateEvaluatorFactory.java:79-81), the Pattern compiled with CASE_INSENSITIVE | UNICODE_CASE
// (RegexpLikePredicate.java:49).  A find() that only has to say yes or no is a regular language of the value's bytes,
// so the device form is a DFA over bytes: a byte -> class map, a next[state][class] table, a start state and an accept
// bit per state.  The accept state is absorbing (a match found stays found).  `^` is folded into the start state.  `$`
// holds at the end of the value and before one final line terminator; the walker knows that place from the value's
// last bytes and feeds the zero-width pseudo-class MARK there and again at the end, and next[s][MARK] is s plus what s
// reaches through `$` edges.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PH_REGEX_HD __host__ __device__
#else
#define PH_REGEX_HD
#endif

namespace ph {

constexpr int kRegexMaxStates = 255;   // DFA states (a state is one byte of the table)
constexpr int kRegexMaxClasses = 64;   // byte classes, MARK included
constexpr int kRegexMaxNfa = 1024;     // nodes of the byte-level NFA the DFA is built from

struct RegexHeader {
  uint8_t cls[256];    // byte -> class
  uint32_t accept[8];  // bit s: state s accepts
  int32_t nstates;
  int32_t nclasses;    // the row length of next (MARK is class nclasses - 1)
  int32_t start;
  int32_t mark;
};

struct RegexProgram {
  RegexHeader h;
  uint8_t next[kRegexMaxStates * kRegexMaxClasses];  // next[s * nclasses + c]; only nstates rows are used
};

// the bytes of a program that are in use, rounded to whole 16-byte chunks (what travels to the device and to LDS)
inline uint32_t regex_program_bytes(const RegexProgram& P) {
  return (uint32_t)(sizeof(RegexHeader) + ((size_t)P.h.nstates * (size_t)P.h.nclasses + 15) / 16 * 16);
}

// A row is read a dword at a time: Row::dword(i) is bytes 4i .. 4i + 3, little endian.  Bytes at or past `width` in the
// last dword are padding that may hold anything; neither function looks at them.
template <class Row>
PH_REGEX_HD inline uint32_t regex_row_byte(const Row& v, int i) {
  return (v.dword(i >> 2) >> (8 * (i & 3))) & 0xFFu;
}

// the value's length: its first zero byte, or width
template <class Row>
PH_REGEX_HD inline int regex_row_len(const Row& v, int width) {
  for (int i = 0; i < width; i += 4) {
    uint32_t w = v.dword(i >> 2);
    if (width - i < 4) w |= 0xFFFFFFFFu << (8 * (width - i));  // padding counts as non-zero
    const uint32_t z = (w - 0x01010101u) & ~w & 0x80808080u;   // its lowest set bit marks the first zero byte
    if (z) return i + (__builtin_ctz(z) >> 3);
  }
  return width;
}

// where `$` holds besides len: before one final line terminator (\r\n is one), -1 when the value does not end in one
template <class Row>
PH_REGEX_HD inline int regex_dollar_place(const Row& v, int len) {
  if (len < 1) return -1;
  const uint32_t c = regex_row_byte(v, len - 1);
  if (c == '\n') return (len >= 2 && regex_row_byte(v, len - 2) == '\r') ? len - 2 : len - 1;
  if (c == '\r') return len - 1;
  if (c == 0x85u && len >= 2 && regex_row_byte(v, len - 2) == 0xC2u) return len - 2;
  if ((c | 1u) == 0xA9u && len >= 3 && regex_row_byte(v, len - 2) == 0x80u && regex_row_byte(v, len - 3) == 0xE2u)
    return len - 3;
  return -1;
}

// the bytes of the dword w (bytes i .. i + 3 of the value) that lie before len, through the DFA from state s
PH_REGEX_HD inline uint32_t regex_feed_dword(uint32_t s, uint32_t w, int i, int len, int dollar, const RegexHeader& h,
                                             const uint8_t* next) {
  const uint32_t nc = (uint32_t)h.nclasses, mark = (uint32_t)h.mark;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i + k < len) {
      if (i + k == dollar) s = next[s * nc + mark];
      s = next[s * nc + h.cls[(w >> (8 * k)) & 0xFFu]];
    }
  }
  return s;
}

PH_REGEX_HD inline bool regex_accepts(uint32_t s, const RegexHeader& h) { return (h.accept[s >> 5] >> (s & 31u)) & 1u; }

// Matcher.find() of the pattern P was compiled from, on the value v[0, len)
template <class Row>
PH_REGEX_HD inline bool regex_match(const Row& v, int len, const RegexProgram& P) {
  const int dollar = regex_dollar_place(v, len);
  uint32_t s = (uint32_t)P.h.start;
  for (int i = 0; i < len; i += 4) s = regex_feed_dword(s, v.dword(i >> 2), i, len, dollar, P.h, P.next);
  s = P.next[s * (uint32_t)P.h.nclasses + (uint32_t)P.h.mark];
  return regex_accepts(s, P.h);
}

}  // namespace ph
