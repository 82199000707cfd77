// mean|a - b|'s per-pixel arithmetic, shared by the stand-alone loss kernels (loss.hip) and the fused forward's
// epilogue (raster_forward.hip, k_raster<..., L1>): both must produce the same sign codes bit for bit and the same
// |d| terms, whatever d is (NaN, +-0, infinities).
#pragma once
#include <hip/hip_runtime.h>

namespace mr {

// 2-bit sign code of d, two's complement: 0 -> 0, 1 -> +1, 3 -> -1 (NaN -> 0, like (0 < d) - (d < 0)); a
// reader gets the value with one signed bit-field extract (v_bfe_i32) and a conversion.
__device__ __forceinline__ unsigned sign_code(float d) { return d > 0.f ? 1u : (d < 0.f ? 3u : 0u); }

// one RGBA pixel's four codes, channel c in bits 2c .. 2c + 1: the byte the loss stores per pixel
__device__ __forceinline__ unsigned sign_code4(float d0, float d1, float d2, float d3) {
  return sign_code(d0) | (sign_code(d1) << 2) | (sign_code(d2) << 4) | (sign_code(d3) << 6);
}

// one RGBA pixel's contribution to sum |a - b|, in the grouping every kernel of the loss uses
__device__ __forceinline__ float abs_sum4(float d0, float d1, float d2, float d3) {
  return (fabsf(d0) + fabsf(d1)) + (fabsf(d2) + fabsf(d3));
}

}  // namespace mr
