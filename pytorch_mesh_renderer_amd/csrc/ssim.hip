// Fused structural-similarity (SSIM, Wang et al. 2004) image loss for gfx950 (MI355X).
//
// In eager torch the mean SSIM of two [B,H,W,C] images is five grouped convolutions, a chain of elementwise passes,
// autograd's saved copies of all of it and the same again backward: well over twenty passes over the image.  Here it
// is one stencil pass each way.
//
//   forward   one workgroup per 32 x 16 tile of the SSIM map.  The tile plus a halo of r = (window - 1) / 2 pixels of
//             both images goes into LDS, one plane per channel (16-byte loads for C = 4); per channel the separable
//             Gaussian blur of x, y, x^2, y^2, xy runs as a row pass into a second LDS array and a column pass out
//             of it; the map value and the derivative terms of the backward are formed in registers, the map values
//             are summed per workgroup, and everything is written once, 16 bytes per pixel and plane for C = 4.
//             C = 4, gradient to the image: reads 2 x 16 B/px, writes 3 x 16 B/px.
//   backward  the same tiling over the image: dL/dx(q) = (G*A)(q) + 2 x(q) (G*B)(q) + y(q) (G*C)(q), a gather (the
//             blur of the saved planes), no atomics.  C = 4, gradient to the image: reads 3 x 16 (saved) + 2 x 16
//             (images) B/px, writes 16 B/px.
//
// With f = ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sxx + syy + C2)) = A1 A2 / (B1 B2) seen as a function of the
// RAW moments (mx, my, Exx, Eyy, Exy), sxx = Exx - mx^2 and so on:
//   B = df/dExx = df/dEyy = -f / B2          C = df/dExy = 2 A1 / (B1 B2)
//   A = df/dmx = 2 (my (A2 - A1) + mx f (B1 - B2)) / (B1 B2)         (for the target: mx and my exchanged)
// B and C serve both images, so a gradient to both costs one plane more, not three.  The planes carry the 1 / n of
// the mean; the backward multiplies by the upstream scalar it reads on the device.
//
// LDS rows: the input planes have an odd row stride (window + 32), so that the row pass -- a wave's 64 lanes are 8 rows
// x 8 groups of four outputs -- reads 32 different banks per half wave; the blurred rows have stride 33 for the row
// pass's stores, and the column pass reads 32 consecutive floats of ONE row per half wave: no bank conflicts either way
// by this arithmetic (worked by hand per 32-lane half wave; no LDS counter run has been made to confirm it).
// LDS per workgroup at window 11: 35,776 + 17,160 B forward (three workgroups per CU), 17,888 + 13,728 B backward.
#include <math.h>

#include "mr_internal.h"

namespace mr {
namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 16;   // outputs per workgroup: 2 per thread and channel
constexpr int kMaxWindow = 11;
constexpr int kMidStride = kTileW + 1;
static_assert(kTileW * kTileH == 2 * kThreads && kTileW == 32, "the column pass gives thread t column t % 32 and rows 2 (t / 32), + 1");

struct SsimWindow {
  float g[kMaxWindow];   // by value in the kernel arguments: scalar registers after unrolling
};

template <int WS>
struct TileShape {
  static constexpr int kInW = kTileW + WS - 1, kInH = kTileH + WS - 1;
  static constexpr int kInStride = (kInW % 2) ? kInW : kInW + 1;   // odd
};

__device__ __forceinline__ float block_sum(float s, float *s_part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
  if ((threadIdx.x & (kWave - 1)) == 0) s_part[threadIdx.x >> 6] = s;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x == 0)
    for (int w = 0; w < kThreads / kWave; ++w) t += s_part[w];
  return t;   // thread 0 only
}

// One channel of the tile's rows blurred along x: four adjacent outputs per work item from WS + 3 loaded values.
// NQ = 5: the moments of an image pair (x, y, x^2, y^2, xy) from two planes; NQ = 1: one plane as it is.
template <int WS, int NQ>
__device__ __forceinline__ void row_pass_item(const float *__restrict__ px, const float *__restrict__ py,
                                              const SsimWindow &win, float *__restrict__ out, int quantity_stride) {
  float x[WS + 3], y[WS + 3];
#pragma unroll
  for (int i = 0; i < WS + 3; ++i) {
    x[i] = px[i];
    if (NQ == 5) y[i] = py[i];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float m[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) m[q] = 0.f;
#pragma unroll
    for (int k = 0; k < WS; ++k) {
      const float w = win.g[k], xv = x[j + k];
      m[0] = fmaf(w, xv, m[0]);
      if (NQ == 5) {
        const float yv = y[j + k];
        m[1] = fmaf(w, yv, m[1]);
        m[2] = fmaf(w, xv * xv, m[2]);
        m[3] = fmaf(w, yv * yv, m[3]);
        m[4] = fmaf(w, xv * yv, m[4]);
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) out[q * quantity_stride + j] = m[q];
  }
}

// Two vertically adjacent outputs of one column from WS + 1 blurred rows.
template <int WS>
__device__ __forceinline__ void column_pass(const float *__restrict__ col, const SsimWindow &win, float &o0, float &o1) {
  float v[WS + 1];
#pragma unroll
  for (int k = 0; k < WS + 1; ++k) v[k] = col[k * kMidStride];
  o0 = 0.f;
  o1 = 0.f;
#pragma unroll
  for (int k = 0; k < WS; ++k) {
    o0 = fmaf(win.g[k], v[k], o0);
    o1 = fmaf(win.g[k], v[k + 1], o1);
  }
}

// The tile of `src` ([.,Hs,Ws,C], image `img`) whose first pixel is (x0, y0), into one LDS plane per channel; pixels
// outside the array read as zero (the zero padding of "same", and the full correlation of the backward).
template <int WS, bool VEC4>
__device__ __forceinline__ void load_tile(const float *__restrict__ src, int img, int Hs, int Ws, int C, int x0, int y0,
                                          float (*__restrict__ planes)[TileShape<WS>::kInH][TileShape<WS>::kInStride]) {
  using Shape = TileShape<WS>;
  for (int i = (int)threadIdx.x; i < Shape::kInH * Shape::kInW; i += kThreads) {
    const int ly = i / Shape::kInW, lx = i - ly * Shape::kInW;
    const int y = y0 + ly, x = x0 + lx;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (y >= 0 && y < Hs && x >= 0 && x < Ws) {
      const size_t p = ((size_t)img * Hs + y) * Ws + x;
      if (VEC4) {
        const float4 t = ((const float4 *)src)[p];
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < C) v[c] = src[p * C + c];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (VEC4 || c < C) planes[c][ly][lx] = v[c];
  }
}

// One pixel's channels (values v[c][.]) to dst[p]: 16 bytes for C = 4.
template <bool VEC4>
__device__ __forceinline__ void store_pixel(float *__restrict__ dst, size_t p, int C, float v0, float v1, float v2,
                                            float v3) {
  if (VEC4) {
    ((float4 *)dst)[p] = make_float4(v0, v1, v2, v3);
  } else {
    const float v[4] = {v0, v1, v2, v3};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) dst[p * C + c] = v[c];
  }
}

// The map value and the planes of the backward (file comment) from one pixel's raw moments.  Written so that two
// IDENTICAL images give f = 1, A = 0 and C = -2 B exactly, as in exact arithmetic, and the backward then returns an
// exact zero: a1 and b1 (a2 and b2) are formed by the same roundings when mx = my (sxx = syy = sxy), the quotients
// are IEEE divisions (x / x = 1), and nothing here is contracted into an fma except where fmaf says so.
struct SsimTerms {
  float f, b, c, ax, ay;
};
__device__ __forceinline__ SsimTerms ssim_terms(float mx, float my, float exx, float eyy, float exy, float c1, float c2,
                                                float inv_n) {
#pragma clang fp contract(off)
  const float sxx = fmaf(-mx, mx, exx), syy = fmaf(-my, my, eyy), sxy = fmaf(-mx, my, exy);
  const float pxy = mx * my;
  const float a1 = (pxy + pxy) + c1, a2 = (sxy + sxy) + c2;
  const float b1 = (mx * mx + my * my) + c1, b2 = (sxx + syy) + c2;
  const float r1 = a1 / b1, r2 = a2 / b2;
  const float k = (1.f / b2) * inv_n;   // the planes carry the mean's 1 / n
  SsimTerms t;
  t.f = r1 * r2;
  t.b = -(t.f * k);
  t.c = 2.f * (r1 * k);
  const float d1 = a2 - a1, d2 = b1 - b2, s = 2.f * (k / b1);
  t.ax = s * (my * d1 + (mx * t.f) * d2);
  t.ay = s * (mx * d1 + (my * t.f) * d2);
  return t;
}

constexpr int kGradImage = MR_SSIM_GRAD_IMAGE, kGradTarget = MR_SSIM_GRAD_TARGET;

// grid (tiles_x, tiles_y, B) over the map [B,Hm,Wm,C]; map pixel (mx, my) is centred on image pixel (mx + off, my + off).
template <int WS, bool VEC4>
__global__ __launch_bounds__(kThreads) void k_ssim_forward(const float *__restrict__ a, const float *__restrict__ b,
                                                           int H, int W, int C, int Hm, int Wm, int off,
                                                           SsimWindow win, float c1, float c2, float inv_n, int grads,
                                                           float *__restrict__ partials, float *__restrict__ map,
                                                           float *__restrict__ saved, size_t plane) {
  using Shape = TileShape<WS>;
  constexpr int R = (WS - 1) / 2;
  __shared__ float s_in[2][4][Shape::kInH][Shape::kInStride];
  __shared__ float s_mid[5][Shape::kInH][kMidStride];
  __shared__ float s_part[kThreads / kWave];
  const int img = (int)blockIdx.z, mx0 = (int)blockIdx.x * kTileW, my0 = (int)blockIdx.y * kTileH;
  const int nc = VEC4 ? 4 : C;
  load_tile<WS, VEC4>(a, img, H, W, C, mx0 + off - R, my0 + off - R, s_in[0]);
  load_tile<WS, VEC4>(b, img, H, W, C, mx0 + off - R, my0 + off - R, s_in[1]);
  __syncthreads();

  const int col = (int)threadIdx.x % kTileW, row = 2 * ((int)threadIdx.x / kTileW);
  const bool want_saved = saved != nullptr;
  float value[4][2], t_b[4][2], t_c[4][2], t_ax[4][2], t_ay[4][2];
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int j = 0; j < 2; ++j) value[c][j] = t_b[c][j] = t_c[c][j] = t_ax[c][j] = t_ay[c][j] = 0.f;
    if (c >= nc) continue;   // (uniform: the barriers below are reached by all threads or none)
    for (int it = (int)threadIdx.x; it < Shape::kInH * (kTileW / 4); it += kThreads) {
      const int ly = it / (kTileW / 4), xg = it % (kTileW / 4);
      row_pass_item<WS, 5>(&s_in[0][c][ly][4 * xg], &s_in[1][c][ly][4 * xg], win, &s_mid[0][ly][4 * xg],
                           Shape::kInH * kMidStride);
    }
    __syncthreads();
    float m[5][2];
#pragma unroll
    for (int q = 0; q < 5; ++q) column_pass<WS>(&s_mid[q][row][col], win, m[q][0], m[q][1]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const SsimTerms t = ssim_terms(m[0][j], m[1][j], m[2][j], m[3][j], m[4][j], c1, c2, inv_n);
      value[c][j] = t.f;
      if (mx0 + col < Wm && my0 + row + j < Hm) sum += t.f;
      if (want_saved) t_b[c][j] = t.b, t_c[c][j] = t.c, t_ax[c][j] = t.ax, t_ay[c][j] = t.ay;
    }
    __syncthreads();   // s_mid is rewritten by the next channel's row pass
  }

#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int mx = mx0 + col, my = my0 + row + j;
    if (mx >= Wm || my >= Hm) continue;
    const size_t p = ((size_t)img * Hm + my) * Wm + mx;
    if (map) store_pixel<VEC4>(map, p, C, value[0][j], value[1][j], value[2][j], value[3][j]);
    if (want_saved) {
      store_pixel<VEC4>(saved, p, C, t_b[0][j], t_b[1][j], t_b[2][j], t_b[3][j]);
      store_pixel<VEC4>(saved + plane, p, C, t_c[0][j], t_c[1][j], t_c[2][j], t_c[3][j]);
      float *next = saved + 2 * plane;
      if (grads & kGradImage) {
        store_pixel<VEC4>(next, p, C, t_ax[0][j], t_ax[1][j], t_ax[2][j], t_ax[3][j]);
        next += plane;
      }
      if (grads & kGradTarget) store_pixel<VEC4>(next, p, C, t_ay[0][j], t_ay[1][j], t_ay[2][j], t_ay[3][j]);
    }
  }
  const float total = block_sum(sum, s_part);
  if (threadIdx.x == 0)   // summed in a fixed order by k_l1_finish: reproducible bits
    partials[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = total * inv_n;
}

// grid (tiles_x, tiles_y, B) over the image [B,H,W,C]; image pixel (x, y) gathers the map pixels (x - off - R + k, ...).
template <int WS, bool VEC4>
__global__ __launch_bounds__(kThreads) void k_ssim_backward(const float *__restrict__ a, const float *__restrict__ b,
                                                            const float *__restrict__ saved, size_t plane,
                                                            const float *__restrict__ upstream, int H, int W, int C,
                                                            int Hm, int Wm, int off, SsimWindow win, int grads,
                                                            float *__restrict__ da, float *__restrict__ db) {
  using Shape = TileShape<WS>;
  constexpr int R = (WS - 1) / 2;
  __shared__ float s_in[4][Shape::kInH][Shape::kInStride];
  __shared__ float s_mid[4][Shape::kInH][kMidStride];
  const int img = (int)blockIdx.z, x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * kTileH;
  const int nc = VEC4 ? 4 : C;
  const int n_planes = 2 + ((grads & kGradImage) ? 1 : 0) + ((grads & kGradTarget) ? 1 : 0);
  const int col = (int)threadIdx.x % kTileW, row = 2 * ((int)threadIdx.x / kTileW);
  float blurred[4][4][2];   // [plane][channel][output]
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int c = 0; c < 4; ++c) blurred[t][c][0] = blurred[t][c][1] = 0.f;
    if (t >= n_planes) continue;   // (uniform)
    // (every thread is past the previous plane's row pass, the last reader of s_in)
    load_tile<WS, VEC4>(saved + t * plane, img, Hm, Wm, C, x0 - off - R, y0 - off - R, s_in);
    __syncthreads();   // ... and past the previous plane's column pass, the last reader of s_mid
    for (int it = (int)threadIdx.x; it < nc * Shape::kInH * (kTileW / 4); it += kThreads) {
      const int xg = it % (kTileW / 4), rest = it / (kTileW / 4);
      const int ly = rest % Shape::kInH, c = rest / Shape::kInH;
      row_pass_item<WS, 1>(&s_in[c][ly][4 * xg], nullptr, win, &s_mid[c][ly][4 * xg], 0);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < nc) column_pass<WS>(&s_mid[c][row][col], win, blurred[t][c][0], blurred[t][c][1]);
  }

  const float up = upstream[0];   // d loss / d mean, read on the device: no host synchronisation
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int x = x0 + col, y = y0 + row + j;
    if (x >= W || y >= H) continue;
    const size_t p = ((size_t)img * H + y) * W + x;
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, yv[4] = {0.f, 0.f, 0.f, 0.f};
    if (VEC4) {
      const float4 ta = ((const float4 *)a)[p], tb = ((const float4 *)b)[p];
      xv[0] = ta.x, xv[1] = ta.y, xv[2] = ta.z, xv[3] = ta.w;
      yv[0] = tb.x, yv[1] = tb.y, yv[2] = tb.z, yv[3] = tb.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) xv[c] = a[p * C + c], yv[c] = b[p * C + c];
    }
    float ga[4], gb[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma clang fp contract(off)   // (2 x) gB + y gC is an exact zero for identical images: see ssim_terms
      const float gB = blurred[0][c][j], gC = blurred[1][c][j];
      // plane 2 is the image's A when the image wants a gradient, else the target's; plane 3 the target's
      const float gAx = blurred[2][c][j], gAy = (grads & kGradImage) ? blurred[3][c][j] : blurred[2][c][j];
      ga[c] = up * (gAx + ((2.f * xv[c]) * gB + yv[c] * gC));
      gb[c] = up * (gAy + ((2.f * yv[c]) * gB + xv[c] * gC));
    }
    if (da) store_pixel<VEC4>(da, p, C, ga[0], ga[1], ga[2], ga[3]);
    if (db) store_pixel<VEC4>(db, p, C, gb[0], gb[1], gb[2], gb[3]);
  }
}

SsimWindow make_window(int window, float sigma) {
  // g[i] ~ exp(-(i - r)^2 / (2 sigma^2)), normalised to sum 1 in double, then rounded to float
  double g[kMaxWindow], sum = 0.0;
  const double r = 0.5 * (window - 1), s = (double)sigma;
  for (int i = 0; i < window; ++i) {
    g[i] = exp(-((double)i - r) * ((double)i - r) / (2.0 * s * s));
    sum += g[i];
  }
  SsimWindow win;
  for (int i = 0; i < kMaxWindow; ++i) win.g[i] = i < window ? (float)(g[i] / sum) : 0.f;
  return win;
}

inline int map_extent(int n, int window, int padding) { return padding == MR_SSIM_VALID ? n - window + 1 : n; }
inline dim3 tiles(int B, int Hn, int Wn) {
  return dim3((unsigned)((Wn + kTileW - 1) / kTileW), (unsigned)((Hn + kTileH - 1) / kTileH), (unsigned)B);
}

}  // namespace

size_t ssim_partials(int B, int H, int W, int window, int padding) {
  const dim3 g = tiles(B, map_extent(H, window, padding), map_extent(W, window, padding));
  return (size_t)g.x * g.y * g.z;
}

size_t ssim_plane_floats(int B, int H, int W, int C, int window, int padding) {
  return (size_t)B * map_extent(H, window, padding) * map_extent(W, window, padding) * C;
}

#define MR_SSIM_DISPATCH(KERNEL, ...)                                                              \
  {                                                                                                \
    if (vec4) switch (window) {                                                                    \
        case 3: hipLaunchKernelGGL((KERNEL<3, true>), __VA_ARGS__); break;                         \
        case 5: hipLaunchKernelGGL((KERNEL<5, true>), __VA_ARGS__); break;                         \
        case 7: hipLaunchKernelGGL((KERNEL<7, true>), __VA_ARGS__); break;                         \
        case 9: hipLaunchKernelGGL((KERNEL<9, true>), __VA_ARGS__); break;                         \
        default: hipLaunchKernelGGL((KERNEL<11, true>), __VA_ARGS__); break;                       \
      }                                                                                            \
    else switch (window) {                                                                         \
        case 3: hipLaunchKernelGGL((KERNEL<3, false>), __VA_ARGS__); break;                        \
        case 5: hipLaunchKernelGGL((KERNEL<5, false>), __VA_ARGS__); break;                        \
        case 7: hipLaunchKernelGGL((KERNEL<7, false>), __VA_ARGS__); break;                        \
        case 9: hipLaunchKernelGGL((KERNEL<9, false>), __VA_ARGS__); break;                        \
        default: hipLaunchKernelGGL((KERNEL<11, false>), __VA_ARGS__); break;                      \
      }                                                                                            \
  }

int launch_ssim_forward(const float *a, const float *b, int B, int H, int W, int C, int window, float sigma, float c1,
                        float c2, int padding, int grads, float *mean, float *map, float *saved, float *partials,
                        hipStream_t s) {
  const int Hm = map_extent(H, window, padding), Wm = map_extent(W, window, padding);
  const int off = padding == MR_SSIM_VALID ? (window - 1) / 2 : 0;
  const size_t plane = ssim_plane_floats(B, H, W, C, window, padding);
  const SsimWindow win = make_window(window, sigma);
  const dim3 grid = tiles(B, Hm, Wm);
  const bool vec4 = C == 4;
  const float inv_n = (float)(1.0 / (double)plane);
  MR_SSIM_DISPATCH(k_ssim_forward, grid, dim3(kThreads), 0, s, a, b, H, W, C, Hm, Wm, off, win, c1, c2, inv_n, grads,
                   partials, map, saved, plane)
  const int rc = check_launch();
  if (rc != MR_OK) return rc;
  return launch_l1_finish(partials, (int)((size_t)grid.x * grid.y * grid.z), mean, s);
}

int launch_ssim_backward(const float *a, const float *b, const float *saved, const float *upstream, int B, int H, int W,
                         int C, int window, float sigma, int padding, int grads, float *da, float *db, hipStream_t s) {
  const int Hm = map_extent(H, window, padding), Wm = map_extent(W, window, padding);
  const int off = padding == MR_SSIM_VALID ? (window - 1) / 2 : 0;
  const size_t plane = ssim_plane_floats(B, H, W, C, window, padding);
  const SsimWindow win = make_window(window, sigma);
  const dim3 grid = tiles(B, H, W);
  const bool vec4 = C == 4;
  MR_SSIM_DISPATCH(k_ssim_backward, grid, dim3(kThreads), 0, s, a, b, saved, plane, upstream, H, W, C, Hm, Wm, off, win,
                   grads, da, db)
  return check_launch();
}

}  // namespace mr
