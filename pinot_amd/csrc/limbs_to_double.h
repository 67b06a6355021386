// limbs_to_double.h -- one correctly rounded conversion of a multi-limb integer to double, shared by the finish kernels
// of the exact integer moments (scan_moments.hip, scan_comoments.hip, scan_moments4.hip).
#pragma once
#include "scan_kernel.h"

namespace ph {

// an unsigned integer of N 64-bit limbs (x[0] lowest; four in the variance and covariance finishes, five in the fourth
// moments') to double, round-to-nearest-even
template <int N>
__device__ __forceinline__ double m_limbs_to_double(const unsigned long long (&x)[N]) {
  int top = -1;
#pragma unroll
  for (int i = 0; i < N; ++i)
    if (x[i]) top = 64 * i + 63 - __clzll((long long)x[i]);
  if (top < 53) return (double)x[0];  // (exact; also the zero)
  const int shift = top - 52;         // the mantissa is bits [shift, shift + 53)
  // the 64 bits from bit `shift` up (nothing above `top` is set) and the bits below it
  const int li = shift >> 6, off = shift & 63;
  unsigned long long a = 0ull, b = 0ull, below = 0ull;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (k == li) a = x[k];
    if (k == li + 1) b = x[k];
    if (k < li) below |= x[k];
  }
  unsigned long long mant = off ? (a >> off) | (b << (64 - off)) : a;
  const unsigned long long rest = off ? a << (64 - off) : 0ull;  // the bits of limb li below `shift`, left-aligned
  bool round_bit, sticky;
  if (off) {
    round_bit = (rest >> 63) != 0ull;
    sticky = (rest << 1) != 0ull || below != 0ull;
  } else {  // the round bit is the top bit of limb li - 1 (li >= 1 here: shift >= 64)
    unsigned long long prev = 0ull, lower = 0ull;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (k == li - 1) prev = x[k];
      if (k < li - 1) lower |= x[k];
    }
    round_bit = (prev >> 63) != 0ull;
    sticky = (prev << 1) != 0ull || lower != 0ull;
  }
  if (round_bit && (sticky || (mant & 1ull))) mant += 1ull;
  return ldexp((double)mant, shift);  // mant <= 2^53: exact, and so is the scaling
}

}  // namespace ph
