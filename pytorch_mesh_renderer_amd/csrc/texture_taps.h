// Pieces shared by the texture sampling kernels (texture.hip: bilinear; texture_mip.hip: mipmapped trilinear):
// the binary32 tap decision, the tap loads, the bilinear rule (weights, blend, d / d(u, v)), tile geometry, the
// backward's scatter of one level's texel gradients (scatter_level: box reduction, LDS window and seam-aware flush,
// leader-round / per-lane atomic fallback) and two host helpers, the channel dispatch and the deterministic scale.
// Both files are compiled with -ffp-contract=off (Makefile): the tap decision is specified un-fused.
#pragma once

#include <type_traits>

#include "mr_internal.h"
#include "det_fixed.h"

namespace mr {
namespace {

constexpr int kTexThreads = 256;                       // 4 wavefronts
constexpr int kTileW = kWave;                          // backward tile: 64 columns ...
constexpr int kTileRowsPerLane = 4;                    // ... x 16 rows, 4 pixels per lane
constexpr int kTileH = kTileRowsPerLane * (kTexThreads / kWave);
constexpr int kTaps = 4 * kTileRowsPerLane;            // texel contributions per lane
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

// The bilinear rule at an already-located sample: the tap weights, the blend and its d / d(u, v).  The expression
// order is part of the contract (the trilinear sampler with f == 0 is bit-identical to the bilinear one).
struct TapWeights {
  float w00, w01, w10, w11;
};
__device__ __forceinline__ TapWeights tap_weights(const Sample &s) {
  const float gx = 1.0f - s.fx, gy = 1.0f - s.fy;
  return TapWeights{gx * gy, s.fx * gy, gx * s.fy, s.fx * s.fy};
}

template <int C, int BOUND>
__device__ __forceinline__ void bilinear(const float *__restrict__ tex, const Sample &s, int Wt, int Ht, float (&o)[C]) {
  Taps<C, BOUND> t;
  t.load(tex, s, Wt, Ht);
  const TapWeights w = tap_weights(s);
#pragma unroll
  for (int c = 0; c < C; ++c) o[c] = ((w.w00 * t.t00[c] + w.w01 * t.t01[c]) + w.w10 * t.t10[c]) + w.w11 * t.t11[c];
}

// d value / d (u, v), contracted with g
template <int C, int BOUND>
__device__ __forceinline__ void bilinear_duv(const float *__restrict__ tex, const Sample &s, int Wt, int Ht,
                                             const float (&g)[C], float &du, float &dv) {
  Taps<C, BOUND> t;
  t.load(tex, s, Wt, Ht);
  const float gx = 1.0f - s.fx, gy = 1.0f - s.fy;
  du = 0.0f;
  dv = 0.0f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    du += g[c] * (gy * (t.t01[c] - t.t00[c]) + s.fy * (t.t11[c] - t.t10[c]));
    dv += g[c] * (gx * (t.t10[c] - t.t00[c]) + s.fx * (t.t11[c] - t.t01[c]));
  }
  du *= (float)Wt;
  dv *= (float)Ht;
}

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

// what a texel gradient is accumulated in, in LDS and in global memory: float, or det_fixed.h's 64-bit fixed point
template <int MODE>
using Accum = std::conditional_t<MODE == kModeFixed, unsigned long long, float>;

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
__device__ __forceinline__ void global_add(Accum<MODE> *__restrict__ dst, size_t k, float v, float to_fixed, int *overflow) {
  if constexpr (MODE == kModeFloat) atomicAdd(dst + k, v);
  else atomic_add_fixed((long long *)dst + k, v, to_fixed, overflow);
}

// The backward's scatter of one level's texel gradients, for one 64 x 16 pixel tile.  EVERY THREAD OF THE WORKGROUP
// CALLS IT, with uniform Wl, Hl, dst and base: it contains barriers.  Per lane: s[j] / on[j] the located sample of its
// pixel in row j and whether it contributes (s[j] zeroed where it does not), g[j] the gradient those taps carry.
// dst + base: the level's [Hl,Wl,C] gradient, float or fixed point by MODE.  `window` holds WINDOW_BYTES.
//
// The workgroup reduces the tap footprint to a box in UNWRAPPED texel indices (clamped ones under clamp; a tile on the
// wrap seam needs no special case).  When box x C fits the window it accumulates there with LDS atomics and flushes
// with row-contiguous global atomics.  Otherwise (minification, UV discontinuities inside the tile) each wavefront
// pre-reduces equal texel keys for kLeaderRounds ballot / readlane rounds and adds the rest with one global atomic
// per lane and channel.  It ends without a barrier: a caller that reuses window or box_part synchronises first.
template <int C, int BOUND, int MODE, int WINDOW_BYTES>
__device__ __forceinline__ void scatter_level(unsigned long long *window, int (*box_part)[4],
                                              const Sample (&s)[kTileRowsPerLane], const bool (&on)[kTileRowsPerLane],
                                              const float (&g)[kTileRowsPerLane][C], int Wl, int Hl,
                                              Accum<MODE> *__restrict__ dst, size_t base, float to_fixed, int *overflow) {
  const int lane = lane_id(), wave = (int)threadIdx.x / kWave;
  int bx0 = INT_MAX, bx1 = INT_MIN, by0 = INT_MAX, by1 = INT_MIN;
#pragma unroll
  for (int j = 0; j < kTileRowsPerLane; ++j) {
    if (!on[j]) continue;
    bx0 = min(bx0, box_index<BOUND>(s[j].x0, Wl));
    bx1 = max(bx1, box_index<BOUND>(s[j].x0 + 1, Wl));
    by0 = min(by0, box_index<BOUND>(s[j].y0, Hl));
    by1 = max(by1, box_index<BOUND>(s[j].y0 + 1, Hl));
  }
  bx0 = wave_min_i(bx0);
  bx1 = wave_max_i(bx1);
  by0 = wave_min_i(by0);
  by1 = wave_max_i(by1);
  if (lane == 0) {
    box_part[wave][0] = bx0;
    box_part[wave][1] = bx1;
    box_part[wave][2] = by0;
    box_part[wave][3] = by1;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kTexThreads / kWave; ++w) {
    bx0 = min(bx0, box_part[w][0]);
    bx1 = max(bx1, box_part[w][1]);
    by0 = min(by0, box_part[w][2]);
    by1 = max(by1, box_part[w][3]);
  }
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;  // >= 1 each (1 under clamp with Wl or Hl = 1), < 2^26
  constexpr int kCap = WINDOW_BYTES / (int)sizeof(Accum<MODE>);
  if (bx0 > bx1) {
    // nothing of the tile at this level (uniform)
  } else if ((long long)bw * bh * C <= kCap) {
    // LDS window [bh][bw][C]
    Accum<MODE> *win = (Accum<MODE> *)window;
    const int n = bw * bh * C, row = bw * C;
    for (int k = (int)threadIdx.x; k < n; k += kTexThreads) win[k] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kTileRowsPerLane; ++j) {
      if (!on[j]) continue;
      const int xa = box_index<BOUND>(s[j].x0, Wl) - bx0, xb = box_index<BOUND>(s[j].x0 + 1, Wl) - bx0;
      const int ya = box_index<BOUND>(s[j].y0, Hl) - by0, yb = box_index<BOUND>(s[j].y0 + 1, Hl) - by0;
      const TapWeights w = tap_weights(s[j]);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        window_add<MODE>(window, ya * row + xa * C + c, w.w00 * g[j][c], to_fixed, overflow);
        window_add<MODE>(window, ya * row + xb * C + c, w.w01 * g[j][c], to_fixed, overflow);
        window_add<MODE>(window, yb * row + xa * C + c, w.w10 * g[j][c], to_fixed, overflow);
        window_add<MODE>(window, yb * row + xb * C + c, w.w11 * g[j][c], to_fixed, overflow);
      }
    }
    __syncthreads();
    // flush: consecutive threads take consecutive cells of a window row, i.e. of a level row (two segments where
    // the row crosses the wrap seam); untouched cells are skipped
    for (int k = (int)threadIdx.x; k < n; k += kTexThreads) {
      const int r = k / row, rem = k - r * row;
      const int col = rem / C, c = rem - col * C;
      const size_t at = base + ((size_t)tex_index<BOUND>(by0 + r, Hl) * Wl + tex_index<BOUND>(bx0 + col, Wl)) * C + c;
      const Accum<MODE> v = win[k];
      if (v != 0) atomicAdd(dst + at, v);
    }
  } else {
    // fallback: texel keys per contribution, a few leader rounds of wavefront pre-reduction, then per-lane atomics
    int key[kTaps];
    float wt[kTaps];
#pragma unroll
    for (int j = 0; j < kTileRowsPerLane; ++j) {
      const int xa = tex_index<BOUND>(s[j].x0, Wl), xb = tex_index<BOUND>(s[j].x0 + 1, Wl);
      const int ya = tex_index<BOUND>(s[j].y0, Hl), yb = tex_index<BOUND>(s[j].y0 + 1, Hl);
      const TapWeights w = tap_weights(s[j]);
      key[4 * j + 0] = on[j] ? ya * Wl + xa : -1;  // < 2^28: abi.hip
      key[4 * j + 1] = on[j] ? ya * Wl + xb : -1;
      key[4 * j + 2] = on[j] ? yb * Wl + xa : -1;
      key[4 * j + 3] = on[j] ? yb * Wl + xb : -1;
      wt[4 * j + 0] = w.w00;
      wt[4 * j + 1] = w.w01;
      wt[4 * j + 2] = w.w10;
      wt[4 * j + 3] = w.w11;
    }
    bool mine = false;
#pragma unroll
    for (int t = 0; t < kTaps; ++t) mine |= key[t] >= 0;
    unsigned long long pending = __ballot(mine);
    for (int round = 0; pending && round < kLeaderRounds; ++round) {  // wave-uniform
      const int leader = __ffsll((long long)pending) - 1;
      int first = -1;
#pragma unroll
      for (int t = kTaps - 1; t >= 0; --t) first = key[t] >= 0 ? key[t] : first;
      const int K = __builtin_amdgcn_readlane(first, leader);
      float sum[C];
#pragma unroll
      for (int c = 0; c < C; ++c) sum[c] = 0.0f;
#pragma unroll
      for (int t = 0; t < kTaps; ++t) {
        if (key[t] != K) continue;
#pragma unroll
        for (int c = 0; c < C; ++c) sum[c] += wt[t] * g[t / 4][c];
        key[t] = -1;
      }
#pragma unroll
      for (int c = 0; c < C; ++c) sum[c] = wave_sum_f(sum[c]);
      if (lane == leader) {
#pragma unroll
        for (int c = 0; c < C; ++c) global_add<MODE>(dst, base + (size_t)K * C + c, sum[c], to_fixed, overflow);
      }
      mine = false;
#pragma unroll
      for (int t = 0; t < kTaps; ++t) mine |= key[t] >= 0;
      pending = __ballot(mine);
    }
#pragma unroll
    for (int t = 0; t < kTaps; ++t) {
      if (key[t] < 0) continue;
#pragma unroll
      for (int c = 0; c < C; ++c) global_add<MODE>(dst, base + (size_t)key[t] * C + c, wt[t] * g[t / 4][c], to_fixed, overflow);
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------
// The runtime channel (or attribute) count n in 1..4 (abi.hip) as a compile-time constant: f receives
// std::integral_constant<int, n>.
template <class F>
inline auto with_channels(int n, F &&f) {
  switch (n) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

// Deterministic mode's scale for a texture scatter: every contribution is w * dout with w <= 1 (tap weight, times
// level weight), so it comes from the largest |dout| and the number of pixels that sample one texture, and no
// texel's sum can leave the 64-bit range.
inline int launch_texture_det_scale(const float *dout, int tex_batched, int B, int W, int H, int C,
                                    DetBlock *det_block, hipStream_t s) {
  const double per_texture = (double)(tex_batched ? 1 : B) * W * H;
  const float gain = (float)fmax(1.0, per_texture / (double)(1 << 21));
  return launch_det_scale(dout, (size_t)B * W * H * C, gain, det_block, s);
}

}  // namespace
}  // namespace mr
