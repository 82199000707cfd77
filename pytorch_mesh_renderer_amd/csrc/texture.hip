// Bilinear texture sampling of a UV pixel buffer (mr_texture_forward / _backward).
//
// Semantics: INTEGRATION.md, "Texture mapping".  Per pixel: x = fl(fl(u * Wt) - 0.5f), y likewise with v and Ht,
// x0 = floor(x), fx = x - x0; the value is the bilinear blend of the taps (y0, x0) (y0, x0+1) (y0+1, x0)
// (y0+1, x0+1), the tap indices wrapped (modulo the size) or clamped to the edge.  A pixel whose mask is <= 0.5,
// whose u or v is not finite or whose |x| or |y| is >= 2^24 is 0 and passes no gradient.  The tap decision is
// binary32, un-fused: this file is compiled with -ffp-contract=off (Makefile), so that a restatement that rounds x
// and y the same way picks the same four texels.
//
// Forward: one lane per pixel; a workgroup covers a contiguous run of one image's pixels (grid = (runs, B)), so the
// image index and the texture base are wave-uniform.
//
// Backward: a workgroup takes a 64 x 16 pixel tile of one image (one wavefront per row, four rows per lane).  d uv
// is per pixel, in gather form, from the same located sample the scatter then uses.  d tex is a scatter: one call of
// texture_taps.h's scatter_level with the texture's own extents and a 32 KiB LDS window (four workgroups per CU; the
// window, its flush and the fallback are described there).  Deterministic mode (mr_set_deterministic) accumulates
// 64-bit fixed point in LDS and in the workspace (integer adds are order-independent) and converts at the end, NaN
// on overflow.
#include "mr_internal.h"
#include "det_fixed.h"
#include "texture_taps.h"

namespace mr {

extern thread_local int g_deterministic;  // mr_set_deterministic (shade.hip)

namespace {

constexpr int kWindowBytes = 32 * 1024;  // LDS accumulation window (4 workgroups per CU)

struct TexArgs {
  const float *tex;     // [Bt,Ht,Wt,C]
  size_t tex_stride;    // floats per texture: Ht * Wt * C when there is one per image, 0 when shared
  const float2 *uv;     // [B,H,W,2]
  const float *mask;    // [B,H,W] or null
  int Ht, Wt, W, H;
};

// ---- forward ----------------------------------------------------------------------------------------------------
template <int C, int BOUND>
__global__ __launch_bounds__(kTexThreads) void k_tex_forward(TexArgs a, float *__restrict__ out) {
  const int b = (int)blockIdx.y;
  const int hw = a.W * a.H;
  const int p = (int)blockIdx.x * kTexThreads + (int)threadIdx.x;
  if (p >= hw) return;
  const size_t i = (size_t)b * hw + p;
  const float *tex = a.tex + (size_t)b * a.tex_stride;  // wave-uniform
  const float2 q = a.uv[i];
  float o[C];
#pragma unroll
  for (int c = 0; c < C; ++c) o[c] = 0.0f;
  Sample s;
  if ((!a.mask || a.mask[i] > 0.5f) && locate(q, a.Wt, a.Ht, s)) bilinear<C, BOUND>(tex, s, a.Wt, a.Ht, o);
  store_c<C>(out + i * C, o);
}

// ---- backward ---------------------------------------------------------------------------------------------------
template <int C, int BOUND, int MODE>
__global__ __launch_bounds__(kTexThreads) void k_tex_backward(TexArgs a, int tiles_x, const float *__restrict__ dout,
                                                             Accum<MODE> *__restrict__ dtex,  // null: d uv only
                                                             float2 *__restrict__ duv,
                                                             DetBlock *__restrict__ det_block) {
  __shared__ unsigned long long window[kWindowBytes / 8];
  __shared__ int box_part[kTexThreads / kWave][4];
  const int b = (int)blockIdx.y;
  const int lane = lane_id(), wave = (int)threadIdx.x / kWave;
  const int px = ((int)blockIdx.x % tiles_x) * kTileW + lane;
  const int py = ((int)blockIdx.x / tiles_x) * kTileH + wave;  // rows py, py + 4, py + 8, py + 12
  const size_t tex_off = (size_t)b * a.tex_stride;
  const float *tex = a.tex + tex_off;

  Sample s[kTileRowsPerLane];
  bool ok[kTileRowsPerLane];
  float g[kTileRowsPerLane][C];
#pragma unroll
  for (int j = 0; j < kTileRowsPerLane; ++j) {
    const int y = py + j * (kTexThreads / kWave);
    ok[j] = false;
    s[j] = Sample{0, 0, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < C; ++c) g[j][c] = 0.0f;
    if (px >= a.W || y >= a.H) continue;
    const size_t i = ((size_t)b * a.H + y) * a.W + px;
    const float2 q = a.uv[i];
    const bool on = !a.mask || a.mask[i] > 0.5f;
    load_c<C>(dout + i * C, g[j]);
    ok[j] = on && locate(q, a.Wt, a.Ht, s[j]);
    if (duv) {
      float du = 0.0f, dv = 0.0f;
      if (ok[j]) bilinear_duv<C, BOUND>(tex, s[j], a.Wt, a.Ht, g[j], du, dv);
      duv[i] = make_float2(du, dv);
    }
  }
  if (!dtex) return;  // uniform
  const float to_fixed = MODE == kModeFixed ? det_block->to_fixed : 0.0f;
  int *overflow = MODE == kModeFixed ? &det_block->overflow : nullptr;
  scatter_level<C, BOUND, MODE, kWindowBytes>(window, box_part, s, ok, g, a.Wt, a.Ht, dtex, tex_off, to_fixed, overflow);
}

inline size_t tex_floats(int tex_batched, int Ht, int Wt, int C, int B) {
  return (size_t)(tex_batched ? B : 1) * Ht * Wt * C;
}
inline size_t fixed_bytes(int tex_batched, int Ht, int Wt, int C, int B) {
  return align_up(tex_floats(tex_batched, Ht, Wt, C, B) * sizeof(long long), 256);
}

template <int MODE>
int launch_backward(const TexArgs &a, int C, int B, int boundary, const float *dout, Accum<MODE> *dtex, float *duv,
                    DetBlock *det_block, hipStream_t s) {
  const int tiles_x = (a.W + kTileW - 1) / kTileW, tiles_y = (a.H + kTileH - 1) / kTileH;
  const dim3 grid((unsigned)((size_t)tiles_x * tiles_y), (unsigned)B), block(kTexThreads);
  with_channels(C, [&](auto c) {
    constexpr int kC = decltype(c)::value;
    if (boundary == MR_TEXTURE_WRAP)
      hipLaunchKernelGGL((k_tex_backward<kC, MR_TEXTURE_WRAP, MODE>), grid, block, 0, s, a, tiles_x, dout, dtex,
                         (float2 *)duv, det_block);
    else
      hipLaunchKernelGGL((k_tex_backward<kC, MR_TEXTURE_CLAMP, MODE>), grid, block, 0, s, a, tiles_x, dout, dtex,
                         (float2 *)duv, det_block);
  });
  return check_launch();
}

TexArgs make_args(const float *tex, int tex_batched, int Ht, int Wt, int C, const float *uv, const float *mask,
                  int W, int H) {
  TexArgs a{tex, tex_batched ? (size_t)Ht * Wt * C : 0, (const float2 *)uv, mask, Ht, Wt, W, H};
  return a;
}

}  // namespace

size_t texture_backward_ws(int tex_batched, int Ht, int Wt, int C, int B) {
  if (g_deterministic == 0) return 0;
  return fixed_bytes(tex_batched, Ht, Wt, C, B) + kDetBlockBytes;
}

int launch_texture_forward(const float *tex, int tex_batched, int Ht, int Wt, int C, const float *uv,
                           const float *mask, int B, int W, int H, int boundary, float *out, hipStream_t s) {
  if (B == 0) return MR_OK;
  const TexArgs a = make_args(tex, tex_batched, Ht, Wt, C, uv, mask, W, H);
  const dim3 grid((unsigned)(((size_t)W * H + kTexThreads - 1) / kTexThreads), (unsigned)B), block(kTexThreads);
  with_channels(C, [&](auto c) {
    constexpr int kC = decltype(c)::value;
    if (boundary == MR_TEXTURE_WRAP) hipLaunchKernelGGL((k_tex_forward<kC, MR_TEXTURE_WRAP>), grid, block, 0, s, a, out);
    else hipLaunchKernelGGL((k_tex_forward<kC, MR_TEXTURE_CLAMP>), grid, block, 0, s, a, out);
  });
  return check_launch();
}

int launch_texture_backward(const float *dout, const float *tex, int tex_batched, int Ht, int Wt, int C,
                            const float *uv, const float *mask, int B, int W, int H, int boundary, float *dtex,
                            float *duv, void *ws, hipStream_t s) {
  if (B == 0 || (!dtex && !duv)) return MR_OK;
  const TexArgs a = make_args(tex, tex_batched, Ht, Wt, C, uv, mask, W, H);
  const size_t n_tex = tex_floats(tex_batched, Ht, Wt, C, B);
  if (!dtex || g_deterministic == 0) {
    if (dtex && zero_async(dtex, n_tex * sizeof(float), s) != hipSuccess) return check_launch();
    return launch_backward<kModeFloat>(a, C, B, boundary, dout, dtex, duv, nullptr, s);
  }
  // Deterministic: a 64-bit copy of dtex in the workspace, scaled by launch_texture_det_scale
  unsigned long long *fixed = (unsigned long long *)ws;
  DetBlock *det_block = (DetBlock *)((char *)ws + fixed_bytes(tex_batched, Ht, Wt, C, B));
  if (zero_async(fixed, fixed_bytes(tex_batched, Ht, Wt, C, B), s) != hipSuccess) return check_launch();
  int rc = launch_texture_det_scale(dout, tex_batched, B, W, H, C, det_block, s);
  if (rc != MR_OK) return rc;
  rc = launch_backward<kModeFixed>(a, C, B, boundary, dout, fixed, duv, det_block, s);
  if (rc != MR_OK) return rc;
  return launch_det_to_float((const long long *)fixed, det_block, dtex, n_tex, s);
}

}  // namespace mr
