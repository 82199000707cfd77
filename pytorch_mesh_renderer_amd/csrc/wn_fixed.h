// The winding number's fixed-point format (mr_winding_number_forward): everything that knows it lives here.
//
// w = sum_f t_f with |t_f| <= 0.5.  Every float32 term is rounded ONCE to the nearest multiple of 2^-kWnFracBits
// (ties to even) and the rounded terms are added exactly in 64-bit integers.  Integer addition is associative, so the
// sum depends neither on the order of the triangles nor on how their range is cut into splits nor on the batch the
// image sat in: bit-identical whatever the launch shape, without atomics.  (det_fixed.h is the same idea with a scale
// found at run time; here the terms are bounded, so the scale is a constant.)
//   |t_f| 2^40 <= 2^39, so kWnMaxTriangles = 2^24 terms stay within +-2^63.
//   A float32 term below 2^-41 rounds to 0: T 2^-41 is the format's share of the error bound.
// A sum that saw a non-finite term is POISONED: between the splits it travels as kWnPoisoned, a value no sum of
// fewer than 2^24 terms reaches, and comes out as NaN.
//
// The helpers are inline: every translation unit compiles them with its own flags.  None of them holds an expression
// that floating-point contraction could change.
#pragma once

#include <stdint.h>

#include "mr_internal.h"

namespace mr {

constexpr int kWnFracBits = 40;
constexpr int kWnMaxTriangles = 1 << 24;
constexpr long long kWnPoisoned = INT64_MIN;

// t (|t| <= 0.5, not NaN) -> the nearest multiple of 2^-40, ties to even, as an integer count of them.  The product
// (double)t * 2^40 is exact and below 2^51, so adding 1.5 * 2^52 rounds it to an integer in the adder -- the one
// rounding -- and leaves that integer in the low bits of the double.
__device__ __forceinline__ long long wn_to_fixed(float t) {
  constexpr double kShift = 6755399441055744.0;   // 1.5 * 2^52
  const double d = __builtin_fma((double)t, (double)(1ll << kWnFracBits), kShift);
  return __double_as_longlong(d) - 0x4338000000000000ll;   // the bits of kShift
}

// The sum back to float, rounded once: int64 -> float32 to nearest even, then an exact power of two.
__device__ __forceinline__ float wn_to_float(long long fixed) {
  return __ll2float_rn(fixed) * (1.0f / (float)(1ll << kWnFracBits));
}

}  // namespace mr
