// like_match.h -- the compiled form of a LIKE pattern and its matcher over one UTF-8 value, as k_like_dict runs it per
// lane out of LDS (like_dict.hip).
//
// The reference rewrites LIKE to REGEXP_LIKE (RegexpPatternConverterUtils.likeToRegexpLike :43-131) and evaluates it
// with java.util.regex's Matcher.find() on every dictionary value (RegexpLikePredicateEvaluatorFactory.java:79-81), a
// pattern without flags.  What that means for the shapes a LIKE can produce ([^]seg0 .* seg1 .* ... segN [$], every
// segment a run of literals and `.`):
//   `.`  one code point that is no line terminator (\n, \r, U+0085, U+2028, U+2029); so neither `_` nor the gap of a
//        `%` crosses a line terminator, and a match lies inside one "line" of the value
//   `^`  offset 0 only
//   `$`  the end of the value, or just before a final line terminator (\r\n counts as one; not between \r and \n)
// Inside a line the gaps are unconstrained, so no backtracking is needed: an anchored first segment is tried at the
// line's start, an anchored last one backwards from the line's end, every other segment takes its leftmost
// occurrence after the previous one.  Values are well-formed UTF-8 (the segment writer encodes them).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PH_LIKE_HD __host__ __device__
#else
#define PH_LIKE_HD
#endif

namespace ph {

constexpr int kLikeMaxSegs = 8;     // segments (runs between unescaped `%`) a program holds
constexpr int kLikeMaxBytes = 128;  // elements (literal bytes and `_`) over all segments
constexpr int kLikeSegElems = 64;   // elements of one segment (bits of its `_` mask)

struct LikeProgram {
  uint64_t wild[kLikeMaxSegs];  // bit j: element j of the segment is `_`
  uint16_t off[kLikeMaxSegs];   // first element of the segment in elems
  uint16_t len[kLikeMaxSegs];   // its elements
  int32_t nseg;                 // 0: the pattern matches every value
  int32_t anchor_start;         // the first segment starts at offset 0 (`^`)
  int32_t anchor_end;           // the last segment ends at `$`
  int32_t pad;
  uint8_t elems[kLikeMaxBytes];  // literal bytes (0 at a `_`)
};

PH_LIKE_HD inline bool like_is_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }
PH_LIKE_HD inline int like_cp_len(uint32_t b) { return b < 0x80u ? 1 : (b < 0xE0u ? 2 : (b < 0xF0u ? 3 : 4)); }

// bytes of the line terminator that starts at v[i] (i < len), 0 when none does
template <class Row>
PH_LIKE_HD inline int like_term_len(const Row& v, int i, int len) {
  const uint32_t c = v[i];
  if (c == '\n' || c == '\r') return 1;
  if (c == 0xC2u && i + 1 < len && v[i + 1] == 0x85u) return 2;
  if (c == 0xE2u && i + 2 < len && v[i + 1] == 0x80u && (v[i + 2] | 1u) == 0xA9u) return 3;
  return 0;
}

// segment k at v[s ..) inside the line that ends at b: the offset after it, or -1
template <class Row>
PH_LIKE_HD inline int like_seg_fwd(const Row& v, int s, int b, const LikeProgram& P, int k) {
  const uint8_t* e = P.elems + P.off[k];
  const uint64_t w = P.wild[k];
  const int n = P.len[k];
  int i = s;
  for (int j = 0; j < n; ++j) {
    if (i >= b) return -1;
    const uint32_t c = v[i];
    if ((w >> j) & 1u) {
      const int l = like_cp_len(c);
      if (like_is_cont(c) || i + l > b) return -1;
      i += l;
    } else {
      if (c != e[j]) return -1;
      ++i;
    }
  }
  return i;
}

// segment k ending exactly at b and starting at or after a: its start, or -1
template <class Row>
PH_LIKE_HD inline int like_seg_back(const Row& v, int a, int b, const LikeProgram& P, int k) {
  const uint8_t* e = P.elems + P.off[k];
  const uint64_t w = P.wild[k];
  int i = b;
  for (int j = P.len[k] - 1; j >= 0; --j) {
    if (i <= a) return -1;
    if ((w >> j) & 1u) {
      const int end = i;
      --i;
      while (i > a && like_is_cont(v[i])) --i;
      const uint32_t c = v[i];
      if (like_is_cont(c) || i + like_cp_len(c) != end) return -1;
    } else {
      --i;
      if (v[i] != e[j]) return -1;
    }
  }
  return i;
}

// Matcher.find() of the pattern P was compiled from, on the value v[0, len)
template <class Row>
PH_LIKE_HD inline bool like_match(const Row& v, int len, const LikeProgram& P) {
  const int nseg = P.nseg;
  if (nseg == 0) return true;
  // where `$` holds besides len: before one final line terminator
  int dollar = -1;
  if (len >= 1) {
    const uint32_t c = v[len - 1];
    if (c == '\n') dollar = (len >= 2 && v[len - 2] == '\r') ? len - 2 : len - 1;
    else if (c == '\r') dollar = len - 1;
    else if (c == 0x85u && len >= 2 && v[len - 2] == 0xC2u) dollar = len - 2;
    else if ((c | 1u) == 0xA9u && len >= 3 && v[len - 2] == 0x80u && v[len - 3] == 0xE2u) dollar = len - 3;
  }
  int a = 0;
  for (;;) {
    int b = a, t = 0;  // the line [a, b) and its terminator's bytes
    while (b < len && (t = like_term_len(v, b, len)) == 0) ++b;
    const bool end_ok = b == len || b == dollar;
    bool ok = true;
    int cur = a;
    for (int k = 0; k < nseg && ok; ++k) {
      const bool first = k == 0 && P.anchor_start, last = k == nseg - 1 && P.anchor_end;
      if (last) {
        if (!end_ok) {
          ok = false;
        } else if (first) {
          ok = like_seg_fwd(v, cur, b, P, k) == b;
        } else {
          ok = like_seg_back(v, cur, b, P, k) >= 0;
        }
        cur = b;
      } else if (first) {
        cur = like_seg_fwd(v, cur, b, P, k);
        ok = cur >= 0;
      } else {
        int r = -1;
        for (int s = cur; s < b && r < 0; ++s)
          if (!like_is_cont(v[s])) r = like_seg_fwd(v, s, b, P, k);
        cur = r;
        ok = r >= 0;
      }
    }
    if (ok) return true;
    if (P.anchor_start || b >= len) return false;
    a = b + t;
  }
}

}  // namespace ph
