// Pieces shared by the texture sampling kernels (texture.hip: bilinear; texture_mip.hip: mipmapped trilinear):
// the binary32 tap decision, the tap loads, tile geometry and the LDS / global accumulation of one contribution.
// Both files are compiled with -ffp-contract=off (Makefile): the tap decision is specified un-fused.
#pragma once

#include "mr_internal.h"
#include "det_fixed.h"

namespace mr {
namespace {

constexpr int kTexThreads = 256;                       // 4 wavefronts
constexpr int kTileW = kWave;                          // backward tile: 64 columns ...
constexpr int kTileRowsPerLane = 4;                    // ... x 16 rows, 4 pixels per lane
constexpr int kTileH = kTileRowsPerLane * (kTexThreads / kWave);
constexpr int kTaps = 4 * kTileRowsPerLane;            // texel contributions per lane
constexpr int kWindowBytes = 32 * 1024;                // LDS accumulation window (4 workgroups per CU)
constexpr int kLeaderRounds = 8;                       // wavefront pre-reduction rounds before per-lane atomics
constexpr float kMaxCoord = 16777216.0f;               // 2^24
constexpr int kModeFloat = 0, kModeFixed = 1;

struct Sample {
  int x0, y0;
  float fx, fy;
};

// The tap decision in binary32, two roundings and no fused multiply-add.  False: the pixel is skipped (a NaN or
// infinite u or v gives a NaN or infinite x or y, which the same test refuses).
__device__ __forceinline__ bool locate(float2 q, int Wt, int Ht, Sample &s) {
  const float x = q.x * (float)Wt - 0.5f;
  const float y = q.y * (float)Ht - 0.5f;
  if (!(fabsf(x) < kMaxCoord) || !(fabsf(y) < kMaxCoord)) return false;
  const float xf = floorf(x), yf = floorf(y);
  s.x0 = (int)xf;
  s.y0 = (int)yf;
  s.fx = x - xf;  // exact: |x| < 2^24
  s.fy = y - yf;
  return true;
}

template <int BOUND>
__device__ __forceinline__ int tex_index(int i, int n) {
  if (BOUND == MR_TEXTURE_WRAP) {
    const int m = i % n;
    return m < 0 ? m + n : m;
  }
  return min(max(i, 0), n - 1);
}

// the first tap index of the footprint box: unwrapped under wrap, clamped under clamp
template <int BOUND>
__device__ __forceinline__ int box_index(int i, int n) {
  return BOUND == MR_TEXTURE_WRAP ? i : min(max(i, 0), n - 1);
}

template <int C>
__device__ __forceinline__ void load_c(const float *__restrict__ p, float (&t)[C]) {
  if constexpr (C == 4) {
    const float4 v = *(const float4 *)p;  // 16-B aligned: abi.hip
    t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
  } else if constexpr (C == 2) {
    const float2 v = *(const float2 *)p;
    t[0] = v.x; t[1] = v.y;
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = p[c];
  }
}

template <int C>
__device__ __forceinline__ void store_c(float *__restrict__ p, const float (&t)[C]) {
  if constexpr (C == 4) {
    *(float4 *)p = make_float4(t[0], t[1], t[2], t[3]);
  } else if constexpr (C == 2) {
    *(float2 *)p = make_float2(t[0], t[1]);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = t[c];
  }
}

template <int C, int BOUND>
struct Taps {
  float t00[C], t01[C], t10[C], t11[C];
  __device__ __forceinline__ void load(const float *__restrict__ tex, const Sample &s, int Wt, int Ht) {
    const int xa = tex_index<BOUND>(s.x0, Wt), xb = tex_index<BOUND>(s.x0 + 1, Wt);
    const int ya = tex_index<BOUND>(s.y0, Ht), yb = tex_index<BOUND>(s.y0 + 1, Ht);
    load_c<C>(tex + ((size_t)ya * Wt + xa) * C, t00);
    load_c<C>(tex + ((size_t)ya * Wt + xb) * C, t01);
    load_c<C>(tex + ((size_t)yb * Wt + xa) * C, t10);
    load_c<C>(tex + ((size_t)yb * Wt + xb) * C, t11);
  }
};

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);  // fixed butterfly: the same sum on every lane
  return v;
}

// one contribution into the LDS window: float add, or fixed point (det_fixed.h's rule, LDS u64 adds)
template <int MODE>
__device__ __forceinline__ void window_add(unsigned long long *win, int k, float v, float to_fixed, int *overflow) {
  if (MODE == kModeFloat) {
    atomicAdd((float *)win + k, v);
  } else {
    const float x = v * to_fixed;
    if (!(fabsf(x) < 9.0e18f)) {
      atomicOr(overflow, 1);
      return;
    }
    atomicAdd(win + k, (unsigned long long)__float2ll_rn(x));
  }
}

template <int MODE>
__device__ __forceinline__ void global_add(float *__restrict__ dtex, unsigned long long *__restrict__ dtex_fixed,
                                           size_t k, float v, float to_fixed, int *overflow) {
  if (MODE == kModeFloat) atomicAdd(dtex + k, v);
  else atomic_add_fixed((long long *)dtex_fixed + k, v, to_fixed, overflow);
}

}  // namespace
}  // namespace mr
