// Mipmapped trilinear texture sampling (mr_texture_mip_forward / _backward) and the screen-space attribute
// derivatives its level of detail needs (mr_attribute_derivatives).
//
// Semantics: INTEGRATION.md, "Texture mapping".  The pyramid's level l + 1 exists while both extents of level l are
// even; its texel is fl(fl(fl(a + b) + fl(c + d)) * 0.25f) of the 2 x 2 block below.  Per pixel the level of detail
// comes from uv_da (the UV step per output pixel), lod = 0.5 log2(rho^2) clamped to [0, L - 1]; the value is the
// bilinear sample (texture_taps.h: the same tap decision, per level with the level's extents) of level l0 =
// floor(lod), blended with level l0 + 1 by f = lod - l0 when f > 0.  This file is compiled with -ffp-contract=off.
//
// Levels >= 1 of one texture lie back to back in one packed buffer; level l starts mip_offset(Ht Wt, l) texels in,
// a closed form (a geometric sum), so a lane needs no table for its own l0.
//
//   k_mip_build         one lane per texel of level l + 1, one launch per level (each reads the one before).
//   k_tex_mip_forward   one lane per pixel, grid (runs, B), like k_tex_forward.
//   k_tex_mip_backward  k_tex_backward's 64 x 16 tile.  d uv per pixel in gather form.  d tex is scattered into a
//                       gradient pyramid, ONE PASS PER LEVEL PRESENT IN THE TILE: for each level one call of
//                       texture_taps.h's scatter_level (k_tex_backward's pass) with the level's extents, its
//                       pixels' samples located at that level and dout times the level weight.  The window is
//                       60 KiB here (a tile's box at its own l0 is up to ~130 x 34 texels: 13k floats at C = 3),
//                       two workgroups per CU.
//   k_mip_fold          one lane per level-0 texel: Horner from the coarsest level down, v = g_l + 0.25f v, which is
//                       dlevel_l[i,j] += 0.25f dlevel_{l+1}[i/2,j/2] applied coarsest first, gathered, no atomics;
//                       in deterministic mode it reads the fixed-point sums and converts them on the way.
#include "mr_internal.h"
#include "det_fixed.h"
#include "texture_taps.h"

namespace mr {

extern thread_local int g_deterministic;  // mr_set_deterministic (shade.hip)

namespace {

constexpr int kMipWindowBytes = 60 * 1024;  // LDS accumulation window (2 workgroups per CU)

// texels before level l >= 1 in the packed pyramid of a texture of n0 texels: n0 (1/4 + ... + 1/4^(l-1)).  Exact:
// 4^(l-1) divides n0 for every level that exists, and 3 divides 4^k - 1.  l = L gives the pyramid's size.
__host__ __device__ inline size_t mip_offset(size_t n0, int l) { return (n0 - (n0 >> (2 * (l - 1)))) / 3; }
// texels per texture in the packed buffer: the pyramid's size rounded up to 4, which keeps every texture's levels
// 16-byte aligned for any C (every level but the last has a multiple of 4 texels)
inline size_t mip_stride(size_t n0, int L) { return (mip_offset(n0, L) + 3) & ~(size_t)3; }

struct MipArgs {
  const float *tex;     // level 0: [Bt,Ht,Wt,C]
  size_t tex_stride;    // floats per texture, 0 when shared
  const float *pyr;     // levels >= 1, packed: [Bt, mip_stride(Ht Wt, L), C]
  size_t pyr_stride;    // floats per texture, 0 when shared
  const float2 *uv;     // [B,H,W,2]
  const float4 *uv_da;  // [B,H,W,4]: du/dX du/dY dv/dX dv/dY
  const float *mask;    // [B,H,W] or null
  int Ht, Wt, W, H, L;
};

template <int C>
__device__ __forceinline__ const float *level_ptr(const float *tex, const float *pyr, size_t n0, int l) {
  return l == 0 ? tex : pyr + mip_offset(n0, l) * C;
}

// lod = 0.5 log2(max(ax^2, ay^2)) in level-0 texels, NaN -> 0, clamped to [0, L - 1]; l0 = floor, f = fraction
__device__ __forceinline__ void level_of_detail(float4 da, int Wt, int Ht, int L, int &l0, float &f) {
  const float ux = da.x * (float)Wt, uy = da.y * (float)Wt, vx = da.z * (float)Ht, vy = da.w * (float)Ht;
  const float ax2 = ux * ux + vx * vx, ay2 = uy * uy + vy * vy;
  float lod = 0.0f;
  if (ax2 == ax2 && ay2 == ay2) lod = 0.5f * log2f(fmaxf(ax2, ay2));  // a NaN derivative: lod 0
  lod = fminf(fmaxf(lod, 0.0f), (float)(L - 1));
  const float fl = floorf(lod);
  l0 = (int)fl;
  f = lod - fl;
}

// the bilinear rule (texture_taps.h) at one level
template <int C, int BOUND>
__device__ __forceinline__ void level_value(const float *__restrict__ lvl, float2 q, int Wl, int Hl, float (&o)[C]) {
  Sample s;
  if (locate(q, Wl, Hl, s)) {
    bilinear<C, BOUND>(lvl, s, Wl, Hl, o);
  } else {  // cannot happen below a level 0 that passed: |x| shrinks with the level
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = 0.0f;
  }
}

// its d value / d (u, v), contracted with g
template <int C, int BOUND>
__device__ __forceinline__ void level_duv(const float *__restrict__ lvl, float2 q, int Wl, int Hl, const float (&g)[C],
                                          float &du, float &dv) {
  du = 0.0f;
  dv = 0.0f;
  Sample s;
  if (locate(q, Wl, Hl, s)) bilinear_duv<C, BOUND>(lvl, s, Wl, Hl, g, du, dv);
}

// ---- pyramid ----------------------------------------------------------------------------------------------------
// two horizontally adjacent texels, 2 C floats at an 8 C-byte aligned address
template <int C>
__device__ __forceinline__ void load_pair(const float *__restrict__ p, float (&v)[2 * C]) {
  if constexpr (C % 2 == 0) {
#pragma unroll
    for (int k = 0; k < C / 2; ++k) {
      const float4 t = ((const float4 *)p)[k];
      v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const float2 t = ((const float2 *)p)[k];
      v[2 * k] = t.x; v[2 * k + 1] = t.y;
    }
  }
}

// dst [Bt, Hd, Wd, C] (Wd = Ws / 2) from src [Bt, 2 Hd, Ws, C]
template <int C>
__global__ __launch_bounds__(kTexThreads) void k_mip_build(const float *__restrict__ src, size_t src_stride,
                                                          float *__restrict__ dst, size_t dst_stride, int Ws, int Wd,
                                                          int n_dst) {
  const int t = (int)blockIdx.x * kTexThreads + (int)threadIdx.x;
  if (t >= n_dst) return;
  const int i = t / Wd, j = t - i * Wd;
  const float *s = src + (size_t)blockIdx.y * src_stride + ((size_t)(2 * i) * Ws + 2 * j) * C;
  float ab[2 * C], cd[2 * C], o[C];
  load_pair<C>(s, ab);
  load_pair<C>(s + (size_t)Ws * C, cd);
#pragma unroll
  for (int c = 0; c < C; ++c) o[c] = ((ab[c] + ab[C + c]) + (cd[c] + cd[C + c])) * 0.25f;
  store_c<C>(dst + (size_t)blockIdx.y * dst_stride + (size_t)t * C, o);
}

// ---- forward ----------------------------------------------------------------------------------------------------
template <int C, int BOUND>
__global__ __launch_bounds__(kTexThreads) void k_tex_mip_forward(MipArgs a, float *__restrict__ out) {
  const int b = (int)blockIdx.y;
  const int hw = a.W * a.H;
  const int p = (int)blockIdx.x * kTexThreads + (int)threadIdx.x;
  if (p >= hw) return;
  const size_t i = (size_t)b * hw + p;
  const float *tex = a.tex + (size_t)b * a.tex_stride;  // wave-uniform
  const float *pyr = a.pyr + (size_t)b * a.pyr_stride;
  const size_t n0 = (size_t)a.Ht * a.Wt;
  const float2 q = a.uv[i];
  float o[C];
#pragma unroll
  for (int c = 0; c < C; ++c) o[c] = 0.0f;
  Sample s0;
  if ((!a.mask || a.mask[i] > 0.5f) && locate(q, a.Wt, a.Ht, s0)) {  // the skip rule, at level 0
    int l0;
    float f;
    level_of_detail(a.uv_da[i], a.Wt, a.Ht, a.L, l0, f);
    level_value<C, BOUND>(level_ptr<C>(tex, pyr, n0, l0), q, a.Wt >> l0, a.Ht >> l0, o);
    if (f > 0.0f) {  // (then l0 + 1 <= L - 1: the clamp)
      float o1[C];
      level_value<C, BOUND>(level_ptr<C>(tex, pyr, n0, l0 + 1), q, a.Wt >> (l0 + 1), a.Ht >> (l0 + 1), o1);
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = (1.0f - f) * o[c] + f * o1[c];
    }
  }
  store_c<C>(out + i * C, o);
}

// ---- backward ---------------------------------------------------------------------------------------------------
// g0 / g1: the gradient pyramid's level 0 [Bt,Ht,Wt,C] and packed levels >= 1, float or 64-bit fixed point by MODE
// (strides in elements per texture, 0 when shared); both null: d uv only
template <int C, int BOUND, int MODE>
__global__ __launch_bounds__(kTexThreads) void k_tex_mip_backward(MipArgs a, int tiles_x,
                                                                 const float *__restrict__ dout,
                                                                 Accum<MODE> *__restrict__ g0, size_t g0_stride,
                                                                 Accum<MODE> *__restrict__ g1, size_t g1_stride,
                                                                 float2 *__restrict__ duv,
                                                                 DetBlock *__restrict__ det_block) {
  __shared__ unsigned long long window[kMipWindowBytes / 8];
  __shared__ int box_part[kTexThreads / kWave][4];
  __shared__ int lvl_part[kTexThreads / kWave][2];
  const int b = (int)blockIdx.y;
  const int lane = lane_id(), wave = (int)threadIdx.x / kWave;
  const int px = ((int)blockIdx.x % tiles_x) * kTileW + lane;
  const int py = ((int)blockIdx.x / tiles_x) * kTileH + wave;  // rows py, py + 4, py + 8, py + 12
  const float *tex = a.tex + (size_t)b * a.tex_stride;
  const float *pyr = a.pyr + (size_t)b * a.pyr_stride;
  const size_t n0 = (size_t)a.Ht * a.Wt;

  float2 q[kTileRowsPerLane];
  bool ok[kTileRowsPerLane];
  int l0[kTileRowsPerLane];
  float f[kTileRowsPerLane];
  float g[kTileRowsPerLane][C];
  int lmin = INT_MAX, lmax = INT_MIN;
#pragma unroll
  for (int j = 0; j < kTileRowsPerLane; ++j) {
    const int y = py + j * (kTexThreads / kWave);
    ok[j] = false;
    q[j] = make_float2(0.0f, 0.0f);
    l0[j] = 0;
    f[j] = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) g[j][c] = 0.0f;
    if (px >= a.W || y >= a.H) continue;
    const size_t i = ((size_t)b * a.H + y) * a.W + px;
    q[j] = a.uv[i];
    const bool on = !a.mask || a.mask[i] > 0.5f;
    load_c<C>(dout + i * C, g[j]);
    Sample s0;
    ok[j] = on && locate(q[j], a.Wt, a.Ht, s0);
    if (ok[j]) {
      level_of_detail(a.uv_da[i], a.Wt, a.Ht, a.L, l0[j], f[j]);
      lmin = min(lmin, l0[j]);
      lmax = max(lmax, f[j] > 0.0f ? l0[j] + 1 : l0[j]);
    }
    if (duv) {
      float du = 0.0f, dv = 0.0f;
      if (ok[j]) {
        level_duv<C, BOUND>(level_ptr<C>(tex, pyr, n0, l0[j]), q[j], a.Wt >> l0[j], a.Ht >> l0[j], g[j], du, dv);
        if (f[j] > 0.0f) {
          float du1, dv1;
          level_duv<C, BOUND>(level_ptr<C>(tex, pyr, n0, l0[j] + 1), q[j], a.Wt >> (l0[j] + 1), a.Ht >> (l0[j] + 1),
                              g[j], du1, dv1);
          du = (1.0f - f[j]) * du + f[j] * du1;
          dv = (1.0f - f[j]) * dv + f[j] * dv1;
        }
      }
      duv[i] = make_float2(du, dv);
    }
  }
  if (!g0) return;  // uniform

  // the levels present in the tile
  lmin = wave_min_i(lmin);
  lmax = wave_max_i(lmax);
  if (lane == 0) {
    lvl_part[wave][0] = lmin;
    lvl_part[wave][1] = lmax;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kTexThreads / kWave; ++w) {
    lmin = min(lmin, lvl_part[w][0]);
    lmax = max(lmax, lvl_part[w][1]);
  }
  if (lmin > lmax) return;  // nothing sampled in the tile (uniform)

  const float to_fixed = MODE == kModeFixed ? det_block->to_fixed : 0.0f;
  int *overflow = MODE == kModeFixed ? &det_block->overflow : nullptr;

  for (int l = lmin; l <= lmax; ++l) {  // uniform: one pass per level
    const int Wl = a.Wt >> l, Hl = a.Ht >> l;
    Accum<MODE> *G = l == 0 ? g0 : g1;
    const size_t base = l == 0 ? (size_t)b * g0_stride : (size_t)b * g1_stride + mip_offset(n0, l) * C;

    Sample s[kTileRowsPerLane];
    bool on[kTileRowsPerLane];
    float gl[kTileRowsPerLane][C];  // level weight x dout
#pragma unroll
    for (int j = 0; j < kTileRowsPerLane; ++j) {
      const bool lower = l0[j] == l, upper = l0[j] + 1 == l && f[j] > 0.0f;
      s[j] = Sample{0, 0, 0.0f, 0.0f};
      on[j] = ok[j] && (lower || upper) && locate(q[j], Wl, Hl, s[j]);
      const float lw = lower ? 1.0f - f[j] : f[j];
#pragma unroll
      for (int c = 0; c < C; ++c) gl[j][c] = lw * g[j][c];
    }
    scatter_level<C, BOUND, MODE, kMipWindowBytes>(window, box_part, s, on, gl, Wl, Hl, G, base, to_fixed, overflow);
    __syncthreads();  // the next level's pass reuses box_part and the window
  }
}

// dtex [Bt,Ht,Wt,C] = level 0 of the folded gradient pyramid (dtex may be g0 itself: a lane reads its own texel)
template <int C, int MODE>
__global__ __launch_bounds__(kTexThreads) void k_mip_fold(const void *g0, const void *__restrict__ g1, size_t g1_stride,
                                                         const DetBlock *__restrict__ det_block, int Ht, int Wt, int L,
                                                         float *dtex) {
  const size_t n0 = (size_t)Ht * Wt;
  const size_t t = (size_t)blockIdx.x * kTexThreads + threadIdx.x;
  if (t >= n0) return;
  const int i = (int)(t / (unsigned)Wt), j = (int)(t - (size_t)i * Wt);
  float v[C];
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = 0.0f;
  for (int l = L - 1; l >= 0; --l) {  // coarsest first
    const size_t at = l == 0 ? (size_t)blockIdx.y * n0 * C + t * C
                             : (size_t)blockIdx.y * g1_stride + (mip_offset(n0, l) + (size_t)(i >> l) * (Wt >> l) + (j >> l)) * C;
    const void *G = l == 0 ? g0 : g1;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float r = MODE == kModeFloat ? ((const float *)G)[at + c] : det_to_float(((const long long *)G)[at + c], det_block);
      v[c] = r + 0.25f * v[c];
    }
  }
  store_c<C>(dtex + (size_t)blockIdx.y * n0 * C + t * C, v);
}

// ---- screen-space attribute derivatives -------------------------------------------------------------------------
// b_i = e_i / s with e_i = U[3i] px + U[3i+1] py + U[3i+2], s = e0 + e1 + e2, U the sign-corrected adjugate of the
// triangle's (x, y, w) matrix, (px, py) the pixel centre in NDC: all formed as the forward rasterizer forms them
// (raster_forward.hip k_setup; un-fused binary32).  One pixel step moves px by
// 2 / W, py by 2 / H.  out [B,H,W,A,2]: (d a / d X, d a / d Y); 0 on the background (interp_fused.hip's test).
template <int A>
__global__ __launch_bounds__(kTexThreads) void k_attr_derivatives(
    const int32_t *__restrict__ ids, const float *__restrict__ bary, const float4 *__restrict__ clip,
    const int32_t *__restrict__ tris, const float *__restrict__ attrs, const int32_t *__restrict__ attr_tris, int V,
    int T, int Va, int W, int H, float2 *__restrict__ out) {
  const int b = (int)blockIdx.y;
  const int hw = W * H;
  const int p = (int)blockIdx.x * kTexThreads + (int)threadIdx.x;
  if (p >= hw) return;
  const size_t pix = (size_t)b * hw + p;
  float2 o[A];
#pragma unroll
  for (int k = 0; k < A; ++k) o[k] = make_float2(0.0f, 0.0f);
  const int t = ids[pix];
  const float b0 = bary[pix * 3], b1 = bary[pix * 3 + 1], b2 = bary[pix * 3 + 2];
  const float pre = (2.0f * b0 + 2.0f * b1) + 2.0f * b2;
  bool covered = pre > 0.0f && (unsigned)t < (unsigned)T;
  int vi[3] = {0, 0, 0}, ai[3] = {0, 0, 0};
  if (covered) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      vi[k] = tris[3 * t + k];
      ai[k] = attr_tris ? attr_tris[3 * t + k] : vi[k];
      covered = covered && (unsigned)vi[k] < (unsigned)V && (unsigned)ai[k] < (unsigned)Va;
    }
  }
  if (covered) {
    const float4 p0 = clip[(size_t)b * V + vi[0]], p1 = clip[(size_t)b * V + vi[1]], p2 = clip[(size_t)b * V + vi[2]];
    const float a11 = p0.x, a12 = p1.x, a13 = p2.x, a21 = p0.y, a22 = p1.y, a23 = p2.y, a31 = p0.w, a32 = p1.w, a33 = p2.w;
    float m[9];
    m[0] = a22 * a33 - a32 * a23; m[1] = a13 * a32 - a33 * a12; m[2] = a12 * a23 - a22 * a13;
    m[3] = a23 * a31 - a33 * a21; m[4] = a11 * a33 - a31 * a13; m[5] = a13 * a21 - a23 * a11;
    m[6] = a21 * a32 - a31 * a22; m[7] = a12 * a31 - a32 * a11; m[8] = a11 * a22 - a21 * a12;
    const float det = a11 * m[0] + a12 * m[3] + a13 * m[6];
    if (det < 0.0f) {
#pragma unroll
      for (int k = 0; k < 9; ++k) m[k] = -m[k];
    }
    const float hw_ = (float)(0.5 * (double)W), hh_ = (float)(0.5 * (double)H);
    const int iy = p / W, ix = p - iy * W;
    const float cx = (float)(((double)ix + 0.5) / (double)hw_ - 1.0);
    const float cy = (float)(((double)iy + 0.5) / (double)hh_ - 1.0);
    const float e0 = m[0] * cx + m[1] * cy + m[2];
    const float e1 = m[3] * cx + m[4] * cy + m[5];
    const float e2 = m[6] * cx + m[7] * cy + m[8];
    const float s = e0 + e1 + e2;
    const float sx = m[0] + m[3] + m[6], sy = m[1] + m[4] + m[7];
    const float kx = 2.0f / (float)W / s, ky = 2.0f / (float)H / s;
    const float cxs[3] = {m[0] - b0 * sx, m[3] - b1 * sx, m[6] - b2 * sx};
    const float cys[3] = {m[1] - b0 * sy, m[4] - b1 * sy, m[7] - b2 * sy};
    const float *base = attrs + (size_t)b * Va * A;
#pragma unroll
    for (int k = 0; k < A; ++k) {
      const float v0 = base[(size_t)ai[0] * A + k], v1 = base[(size_t)ai[1] * A + k], v2 = base[(size_t)ai[2] * A + k];
      o[k].x = ((v0 * cxs[0] + v1 * cxs[1]) + v2 * cxs[2]) * kx;
      o[k].y = ((v0 * cys[0] + v1 * cys[1]) + v2 * cys[2]) * ky;
    }
  }
#pragma unroll
  for (int k = 0; k < A; ++k) out[pix * A + k] = o[k];
}

// ---- host -------------------------------------------------------------------------------------------------------
inline int tz(int v) { return __builtin_ctz((unsigned)v); }

inline size_t count_of(int tex_batched, int B) { return (size_t)(tex_batched ? B : 1); }

MipArgs make_args(const float *tex, const float *pyr, int tex_batched, int Ht, int Wt, int C, int L, const float *uv,
                  const float *uv_da, const float *mask, int W, int H) {
  const size_t n0 = (size_t)Ht * Wt;
  MipArgs a{tex, tex_batched ? n0 * C : 0, pyr, tex_batched ? mip_stride(n0, L) * C : 0, (const float2 *)uv,
            (const float4 *)uv_da, mask, Ht, Wt, W, H, L};
  return a;
}

int launch_build(const float *tex, int tex_batched, int Ht, int Wt, int C, int L, int B, float *pyr, hipStream_t s) {
  const size_t n0 = (size_t)Ht * Wt, count = count_of(tex_batched, B);
  const size_t pyr_stride = mip_stride(n0, L) * C;
  for (int l = 0; l + 1 < L; ++l) {
    const float *src = l == 0 ? tex : pyr + mip_offset(n0, l) * C;
    const size_t src_stride = l == 0 ? n0 * C : pyr_stride;
    const int Ws = Wt >> l, Wd = Wt >> (l + 1), n_dst = Wd * (Ht >> (l + 1));
    const dim3 grid((unsigned)((n_dst + kTexThreads - 1) / kTexThreads), (unsigned)count), block(kTexThreads);
    with_channels(C, [&](auto c) {
      hipLaunchKernelGGL((k_mip_build<decltype(c)::value>), grid, block, 0, s, src, src_stride,
                         pyr + mip_offset(n0, l + 1) * C, pyr_stride, Ws, Wd, n_dst);
    });
    const int rc = check_launch();
    if (rc != MR_OK) return rc;
  }
  return MR_OK;
}

template <int MODE>
int launch_backward(const MipArgs &a, int C, int B, int boundary, const float *dout, Accum<MODE> *g0, size_t g0_stride,
                    Accum<MODE> *g1, size_t g1_stride, float *duv, DetBlock *det_block, hipStream_t s) {
  const int tiles_x = (a.W + kTileW - 1) / kTileW, tiles_y = (a.H + kTileH - 1) / kTileH;
  const dim3 grid((unsigned)((size_t)tiles_x * tiles_y), (unsigned)B), block(kTexThreads);
  with_channels(C, [&](auto c) {
    constexpr int kC = decltype(c)::value;
    if (boundary == MR_TEXTURE_WRAP)
      hipLaunchKernelGGL((k_tex_mip_backward<kC, MR_TEXTURE_WRAP, MODE>), grid, block, 0, s, a, tiles_x, dout, g0,
                         g0_stride, g1, g1_stride, (float2 *)duv, det_block);
    else
      hipLaunchKernelGGL((k_tex_mip_backward<kC, MR_TEXTURE_CLAMP, MODE>), grid, block, 0, s, a, tiles_x, dout, g0,
                         g0_stride, g1, g1_stride, (float2 *)duv, det_block);
  });
  return check_launch();
}

template <int MODE>
int launch_fold(int C, const void *g0, const void *g1, size_t g1_stride, const DetBlock *det_block, int Ht, int Wt,
                int L, size_t count, float *dtex, hipStream_t s) {
  const size_t n0 = (size_t)Ht * Wt;
  const dim3 grid((unsigned)((n0 + kTexThreads - 1) / kTexThreads), (unsigned)count), block(kTexThreads);
  with_channels(C, [&](auto c) {
    hipLaunchKernelGGL((k_mip_fold<decltype(c)::value, MODE>), grid, block, 0, s, g0, g1, g1_stride, det_block, Ht, Wt,
                       L, dtex);
  });
  return check_launch();
}

}  // namespace

int texture_mip_levels(int Ht, int Wt, int max_level) {
  int l = tz(Ht) < tz(Wt) ? tz(Ht) : tz(Wt);
  if (max_level >= 0 && max_level < l) l = max_level;
  return 1 + l;
}

size_t texture_mip_pyramid_floats(int tex_batched, int Ht, int Wt, int C, int B, int L) {
  return count_of(tex_batched, B) * mip_stride((size_t)Ht * Wt, L) * C;
}

size_t texture_mip_backward_ws(int tex_batched, int Ht, int Wt, int C, int B, int L) {
  const size_t count = count_of(tex_batched, B), n0 = (size_t)Ht * Wt, np = mip_stride(n0, L);
  if (g_deterministic == 0) return align_up(count * np * C * sizeof(float), 256);
  return align_up(count * (n0 + np) * C * sizeof(long long), 256) + kDetBlockBytes;
}

int launch_texture_mip_forward(const float *tex, int tex_batched, int Ht, int Wt, int C, int L, const float *uv,
                               const float *uv_da, const float *mask, int B, int W, int H, int boundary, float *pyr,
                               float *out, hipStream_t s) {
  if (B == 0) return MR_OK;
  const int rc = launch_build(tex, tex_batched, Ht, Wt, C, L, B, pyr, s);
  if (rc != MR_OK || !out) return rc;  // out null: the pyramid alone
  const MipArgs a = make_args(tex, pyr, tex_batched, Ht, Wt, C, L, uv, uv_da, mask, W, H);
  const dim3 grid((unsigned)(((size_t)W * H + kTexThreads - 1) / kTexThreads), (unsigned)B), block(kTexThreads);
  with_channels(C, [&](auto c) {
    constexpr int kC = decltype(c)::value;
    if (boundary == MR_TEXTURE_WRAP) hipLaunchKernelGGL((k_tex_mip_forward<kC, MR_TEXTURE_WRAP>), grid, block, 0, s, a, out);
    else hipLaunchKernelGGL((k_tex_mip_forward<kC, MR_TEXTURE_CLAMP>), grid, block, 0, s, a, out);
  });
  return check_launch();
}

int launch_texture_mip_backward(const float *dout, const float *tex, const float *pyr, int tex_batched, int Ht, int Wt,
                                int C, int L, const float *uv, const float *uv_da, const float *mask, int B, int W,
                                int H, int boundary, float *dtex, float *duv, void *ws, hipStream_t s) {
  if (B == 0 || (!dtex && !duv)) return MR_OK;
  const MipArgs a = make_args(tex, pyr, tex_batched, Ht, Wt, C, L, uv, uv_da, mask, W, H);
  const size_t count = count_of(tex_batched, B), n0 = (size_t)Ht * Wt, np = mip_stride(n0, L);
  if (!dtex) return launch_backward<kModeFloat>(a, C, B, boundary, dout, nullptr, 0, nullptr, 0, duv, nullptr, s);
  if (g_deterministic == 0) {
    // level 0 of the gradient pyramid is dtex itself, the packed levels >= 1 are the workspace
    float *g1 = (float *)ws;
    if (zero_async(dtex, count * n0 * C * sizeof(float), s) != hipSuccess) return check_launch();
    if (zero_async(g1, count * np * C * sizeof(float), s) != hipSuccess) return check_launch();
    const int rc = launch_backward<kModeFloat>(a, C, B, boundary, dout, dtex, a.tex_stride, g1, a.pyr_stride, duv,
                                               nullptr, s);
    if (rc != MR_OK || L == 1) return rc;
    return launch_fold<kModeFloat>(C, dtex, g1, np * C, nullptr, Ht, Wt, L, count, dtex, s);
  }
  // Deterministic: the whole gradient pyramid as 64-bit sums in the workspace, scaled by launch_texture_det_scale;
  // the fold converts each level's sums and adds them in a fixed order.
  const size_t fixed_bytes = align_up(count * (n0 + np) * C * sizeof(long long), 256);
  unsigned long long *f0 = (unsigned long long *)ws, *f1 = f0 + count * n0 * C;
  DetBlock *det_block = (DetBlock *)((char *)ws + fixed_bytes);
  if (zero_async(f0, fixed_bytes, s) != hipSuccess) return check_launch();
  int rc = launch_texture_det_scale(dout, tex_batched, B, W, H, C, det_block, s);
  if (rc != MR_OK) return rc;
  rc = launch_backward<kModeFixed>(a, C, B, boundary, dout, f0, a.tex_stride, f1, a.pyr_stride, duv, det_block, s);
  if (rc != MR_OK) return rc;
  return launch_fold<kModeFixed>(C, f0, f1, np * C, det_block, Ht, Wt, L, count, dtex, s);
}

int launch_attribute_derivatives(const int32_t *ids, const float *bary, const float *clip, const int32_t *tris,
                                 const float *attrs, const int32_t *attr_tris, int B, int V, int T, int Va, int W,
                                 int H, int A, float *out, hipStream_t s) {
  if (B == 0) return MR_OK;
  const dim3 grid((unsigned)(((size_t)W * H + kTexThreads - 1) / kTexThreads), (unsigned)B), block(kTexThreads);
  with_channels(A, [&](auto n) {
    hipLaunchKernelGGL((k_attr_derivatives<decltype(n)::value>), grid, block, 0, s, ids, bary, (const float4 *)clip,
                       tris, attrs, attr_tris, V, T, Va, W, H, (float2 *)out);
  });
  return check_launch();
}

}  // namespace mr
