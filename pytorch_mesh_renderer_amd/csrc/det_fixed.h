// The deterministic mode's fixed-point format (mr_set_deterministic): everything that knows it lives here.
//
// Sums are accumulated in 64-bit FIXED POINT with integer atomics.  Integer addition is associative (also
// through two's-complement wrap-around), so the result no longer depends on the order in which lanes and
// wavefronts commit: bit-identical from run to run, where float atomics differ in the last bits.
// DetBlock::to_fixed = 2^k converts to fixed point (a power of two: exact), DetBlock::from_fixed = 2^-k back;
// k is derived on the device from the largest upstream gradient g (DetBlock::max_bits holds its float bits)
// so that g maps to about 2^41: values down to g * 2^-42 are resolved and a triangle's total may reach
// g * 2^21 before the 64-bit range ends.
// A contribution that does not fit -- NaN, infinite, or beyond +-2^63 after scaling (1 / det of a sliver
// triangle times a large upstream gradient) -- is not converted (the conversion of an out-of-range float is
// garbage of arbitrary sign): it raises DetBlock::overflow instead, and det_to_float, through which every sum
// goes back to float, answers NaN for the whole launch when the flag is set -- the float path's answer to such
// inputs, spread over the whole output, instead of a finite wrong number.  (Sums of many in-range
// contributions still wrap silently beyond 2^63: the scale leaves 2^21 of headroom over the largest upstream
// gradient.)
//
// The helpers are static / inline: every translation unit compiles them with its own flags.  None of them
// holds an expression that floating-point contraction could change (single multiplies and integer operations).
#pragma once

#include "mr_internal.h"

namespace mr {

// One per launch, in the pass's workspace, zeroed per launch.
constexpr size_t kDetBlockBytes = 512;
struct DetBlock {
  float to_fixed, from_fixed;  // 2^k, 2^-k
  int max_bits;                // bits of the largest |upstream gradient| (a NaN sorts on top)
  int overflow;                // != 0: a contribution did not fit
  char pad[kDetBlockBytes - 16];
};
static_assert(sizeof(DetBlock) == kDetBlockBytes, "the workspaces reserve kDetBlockBytes");

// (kernels take the block as const __restrict__ for the scale's sake; the flag is the one member they write)
__device__ __forceinline__ int *det_overflow_flag(const DetBlock *block) { return const_cast<int *>(&block->overflow); }

__device__ __forceinline__ void atomic_add_fixed(long long *p, float v, float to_fixed, int *overflow) {
  const float x = v * to_fixed;
  if (!(fabsf(x) < 9.0e18f)) {
    atomicOr(overflow, 1);
    return;
  }
  atomicAdd((unsigned long long *)p, (unsigned long long)__float2ll_rn(x));
}

__device__ __forceinline__ float det_to_float(long long fixed, const DetBlock *block) {
  return block->overflow ? __int_as_float(0x7fc00000) : (float)fixed * block->from_fixed;
}

// max_bits = largest |x[i]|.  RGB_OF_RGBA: x is an RGBA image (n a multiple of 4) whose alpha does not count.
template <bool RGB_OF_RGBA>
static __global__ __launch_bounds__(256) void k_det_abs_max(const float *__restrict__ x, size_t n, DetBlock *__restrict__ block) {
  int best = 0;  // non-negative floats order like integers; a NaN sorts on top
  if (RGB_OF_RGBA) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n / 4; i += (size_t)gridDim.x * 256) {
      const float4 v = ((const float4 *)x)[i];
      best = max(max(best, __float_as_int(fabsf(v.x))), max(__float_as_int(fabsf(v.y)), __float_as_int(fabsf(v.z))));
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
      best = max(best, __float_as_int(fabsf(x[i])));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = max(best, __shfl_down(best, off));
  __shared__ int s_best[4];  // one atomic per WORKGROUP (thousands on one address queue up)
  if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) best = max(best, s_best[w]);
    if (best != 0) atomicMax(&block->max_bits, best);
  }
}

// (2^k, 2^-k) with k such that g = |value| * gain maps to about 2^41; value = scalar[0] * factor, or, with
// scalar == nullptr, the float behind the block's max_bits
static __global__ void k_det_scale(DetBlock *__restrict__ block, const float *__restrict__ scalar, float factor, float gain) {
  const float value = scalar ? scalar[0] * factor : __int_as_float(block->max_bits);
  const float g = fabsf(value) * gain;
  int e = 0;
  if (g > 0.0f && g < INFINITY) (void)frexpf(g, &e);  // g = m * 2^e, m in [0.5, 1)
  const int k = min(max(41 - e, -100), 100);
  block->to_fixed = ldexpf(1.0f, k);
  block->from_fixed = ldexpf(1.0f, -k);
}

// The three ways to a block's scale pair.  gain: the largest factor a contribution may carry over the upstream
// gradient beyond the 2^21 of headroom the scale leaves (1 for the rasterizer / shading passes; 1 / min(sigma,
// gamma) for SoftRas).
// 1. The caller has zeroed the block and a pass of its own has filled max_bits.
inline int launch_det_scale_of_max(DetBlock *block, float gain, hipStream_t s) {
  hipLaunchKernelGGL(k_det_scale, dim3(1), dim3(1), 0, s, block, (const float *)nullptr, 1.0f, gain);
  return check_launch();
}
// 2. Zeroes the block and takes the largest of the n floats at x, the upstream gradient image (rgb_of_rgba: see
//    k_det_abs_max).
inline int launch_det_scale(const float *x, size_t n, float gain, DetBlock *block, hipStream_t s, bool rgb_of_rgba = false) {
  if (zero_async(block, kDetBlockBytes, s) != hipSuccess) return check_launch();
  const size_t want = ((rgb_of_rgba ? n / 4 : n) + 255) / 256;
  const dim3 grid((unsigned)(want < 2048 ? (want ? want : 1) : 2048));
  if (rgb_of_rgba) hipLaunchKernelGGL(k_det_abs_max<true>, grid, dim3(256), 0, s, x, n, block);
  else hipLaunchKernelGGL(k_det_abs_max<false>, grid, dim3(256), 0, s, x, n, block);
  const int rc = check_launch();
  return rc != MR_OK ? rc : launch_det_scale_of_max(block, gain, s);
}
// 3. Zeroes the block; the upstream gradient is one device scalar times a host factor (a mean's: 1 / n) behind
//    sign codes.
inline int launch_det_scale_of_scalar(const float *scalar, float factor, DetBlock *block, hipStream_t s) {
  if (zero_async(block, kDetBlockBytes, s) != hipSuccess) return check_launch();
  hipLaunchKernelGGL(k_det_scale, dim3(1), dim3(1), 0, s, block, scalar, factor, 1.0f);
  return check_launch();
}

// Fixed point back to float: `fixed` holds up to four arrays back to back, array k going to dst[k][0 .. len[k]).
struct DetSegments {
  float *dst[4];
  size_t len[4];
};
static __global__ __launch_bounds__(256) void k_det_to_float(const long long *__restrict__ fixed,
                                                             const DetBlock *__restrict__ block, DetSegments seg, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float v = det_to_float(fixed[i], block);
    size_t at = i;
    bool stored = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (stored) continue;
      if (at < seg.len[k]) {
        seg.dst[k][at] = v;
        stored = true;
      } else {
        at -= seg.len[k];
      }
    }
  }
}
inline int launch_det_to_float(const long long *fixed, const DetBlock *block, const DetSegments &seg, hipStream_t s) {
  const size_t n = seg.len[0] + seg.len[1] + seg.len[2] + seg.len[3];
  if (n == 0) return MR_OK;
  const size_t want = (n + 255) / 256;
  hipLaunchKernelGGL(k_det_to_float, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, s, fixed, block, seg, n);
  return check_launch();
}
inline int launch_det_to_float(const long long *fixed, const DetBlock *block, float *dst, size_t n, hipStream_t s) {
  return launch_det_to_float(fixed, block, DetSegments{{dst, nullptr, nullptr, nullptr}, {n, 0, 0, 0}}, s);
}

}  // namespace mr
