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
// is per pixel, in gather form.  d tex is a scatter: the workgroup finds the tile's tap footprint, a box in
// UNWRAPPED texel indices (a tile on the wrap seam needs no special case), and when box x C fits the LDS window it
// accumulates there with LDS atomics and flushes the window with row-contiguous global atomics (a window row that
// crosses the seam is two segments of the texture row).  Otherwise (minification, UV discontinuities inside the
// tile) each wavefront pre-reduces equal texel keys for a few ballot / readlane leader rounds and adds the rest
// with one global atomic per lane and channel.  Deterministic mode (mr_set_deterministic) accumulates 64-bit fixed
// point in LDS and in the workspace (integer adds are order-independent) and converts at the end, NaN on overflow.
#include "mr_internal.h"
#include "det_fixed.h"
#include "texture_taps.h"

namespace mr {

extern thread_local int g_deterministic;  // mr_set_deterministic (shade.hip)

namespace {

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
  if ((!a.mask || a.mask[i] > 0.5f) && locate(q, a.Wt, a.Ht, s)) {
    Taps<C, BOUND> t;
    t.load(tex, s, a.Wt, a.Ht);
    const float gx = 1.0f - s.fx, gy = 1.0f - s.fy;
    const float w00 = gx * gy, w01 = s.fx * gy, w10 = gx * s.fy, w11 = s.fx * s.fy;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = ((w00 * t.t00[c] + w01 * t.t01[c]) + w10 * t.t10[c]) + w11 * t.t11[c];
  }
  store_c<C>(out + i * C, o);
}

// ---- backward ---------------------------------------------------------------------------------------------------
template <int C, int BOUND, int MODE>
__global__ __launch_bounds__(kTexThreads) void k_tex_backward(TexArgs a, int tiles_x, const float *__restrict__ dout,
                                                             float *__restrict__ dtex,
                                                             unsigned long long *__restrict__ dtex_fixed,
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
  const bool want_tex = MODE == kModeFixed ? dtex_fixed != nullptr : dtex != nullptr;  // uniform

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
      if (ok[j]) {
        Taps<C, BOUND> t;
        t.load(tex, s[j], a.Wt, a.Ht);
        const float gx = 1.0f - s[j].fx, gy = 1.0f - s[j].fy;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          du += g[j][c] * (gy * (t.t01[c] - t.t00[c]) + s[j].fy * (t.t11[c] - t.t10[c]));
          dv += g[j][c] * (gx * (t.t10[c] - t.t00[c]) + s[j].fx * (t.t11[c] - t.t01[c]));
        }
        du *= (float)a.Wt;
        dv *= (float)a.Ht;
      }
      duv[i] = make_float2(du, dv);
    }
  }
  if (!want_tex) return;

  // the tile's tap footprint
  int bx0 = INT_MAX, bx1 = INT_MIN, by0 = INT_MAX, by1 = INT_MIN;
#pragma unroll
  for (int j = 0; j < kTileRowsPerLane; ++j) {
    if (!ok[j]) continue;
    bx0 = min(bx0, box_index<BOUND>(s[j].x0, a.Wt));
    bx1 = max(bx1, box_index<BOUND>(s[j].x0 + 1, a.Wt));
    by0 = min(by0, box_index<BOUND>(s[j].y0, a.Ht));
    by1 = max(by1, box_index<BOUND>(s[j].y0 + 1, a.Ht));
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
  if (bx0 > bx1) return;  // nothing sampled in the tile (uniform)

  const float to_fixed = MODE == kModeFixed ? det_block->to_fixed : 0.0f;
  int *overflow = MODE == kModeFixed ? &det_block->overflow : nullptr;
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;  // >= 1 each (1 under clamp with Wt or Ht = 1), < 2^26
  constexpr int kCap = MODE == kModeFixed ? kWindowBytes / 8 : kWindowBytes / 4;
  if ((long long)bw * bh * C <= kCap) {
    // LDS window [bh][bw][C]
    const int n = bw * bh * C, row = bw * C;
    for (int k = (int)threadIdx.x; k < n; k += kTexThreads) {
      if (MODE == kModeFixed) window[k] = 0ull;
      else ((float *)window)[k] = 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kTileRowsPerLane; ++j) {
      if (!ok[j]) continue;
      const int xa = box_index<BOUND>(s[j].x0, a.Wt) - bx0, xb = box_index<BOUND>(s[j].x0 + 1, a.Wt) - bx0;
      const int ya = box_index<BOUND>(s[j].y0, a.Ht) - by0, yb = box_index<BOUND>(s[j].y0 + 1, a.Ht) - by0;
      const float gx = 1.0f - s[j].fx, gy = 1.0f - s[j].fy;
      const float w00 = gx * gy, w01 = s[j].fx * gy, w10 = gx * s[j].fy, w11 = s[j].fx * s[j].fy;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        window_add<MODE>(window, ya * row + xa * C + c, w00 * g[j][c], to_fixed, overflow);
        window_add<MODE>(window, ya * row + xb * C + c, w01 * g[j][c], to_fixed, overflow);
        window_add<MODE>(window, yb * row + xa * C + c, w10 * g[j][c], to_fixed, overflow);
        window_add<MODE>(window, yb * row + xb * C + c, w11 * g[j][c], to_fixed, overflow);
      }
    }
    __syncthreads();
    // flush: consecutive threads take consecutive floats of a window row, i.e. of a texture row (two segments
    // where the row crosses the wrap seam); untouched cells are skipped
    for (int k = (int)threadIdx.x; k < n; k += kTexThreads) {
      const int r = k / row, rem = k - r * row;
      const int col = rem / C, c = rem - col * C;
      const size_t dst = tex_off + ((size_t)tex_index<BOUND>(by0 + r, a.Ht) * a.Wt + tex_index<BOUND>(bx0 + col, a.Wt)) * C + c;
      if (MODE == kModeFloat) {
        const float v = ((const float *)window)[k];
        if (v != 0.0f) atomicAdd(dtex + dst, v);
      } else {
        const unsigned long long v = window[k];
        if (v != 0ull) atomicAdd(dtex_fixed + dst, v);
      }
    }
    return;
  }

  // fallback: texel keys per contribution, a few leader rounds of wavefront pre-reduction, then per-lane atomics
  int key[kTaps];
  float wt[kTaps];
#pragma unroll
  for (int j = 0; j < kTileRowsPerLane; ++j) {
    const int xa = tex_index<BOUND>(s[j].x0, a.Wt), xb = tex_index<BOUND>(s[j].x0 + 1, a.Wt);
    const int ya = tex_index<BOUND>(s[j].y0, a.Ht), yb = tex_index<BOUND>(s[j].y0 + 1, a.Ht);
    const float gx = 1.0f - s[j].fx, gy = 1.0f - s[j].fy;
    key[4 * j + 0] = ok[j] ? ya * a.Wt + xa : -1;  // < 2^28: abi.hip
    key[4 * j + 1] = ok[j] ? ya * a.Wt + xb : -1;
    key[4 * j + 2] = ok[j] ? yb * a.Wt + xa : -1;
    key[4 * j + 3] = ok[j] ? yb * a.Wt + xb : -1;
    wt[4 * j + 0] = gx * gy;
    wt[4 * j + 1] = s[j].fx * gy;
    wt[4 * j + 2] = gx * s[j].fy;
    wt[4 * j + 3] = s[j].fx * s[j].fy;
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
      for (int c = 0; c < C; ++c) global_add<MODE>(dtex, dtex_fixed, tex_off + (size_t)K * C + c, sum[c], to_fixed, overflow);
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
    for (int c = 0; c < C; ++c)
      global_add<MODE>(dtex, dtex_fixed, tex_off + (size_t)key[t] * C + c, wt[t] * g[t / 4][c], to_fixed, overflow);
  }
}

inline size_t tex_floats(int tex_batched, int Ht, int Wt, int C, int B) {
  return (size_t)(tex_batched ? B : 1) * Ht * Wt * C;
}
inline size_t fixed_bytes(int tex_batched, int Ht, int Wt, int C, int B) {
  return align_up(tex_floats(tex_batched, Ht, Wt, C, B) * sizeof(long long), 256);
}

template <int C>
int launch_forward_c(const TexArgs &a, int B, int boundary, float *out, hipStream_t s) {
  const dim3 grid((unsigned)(((size_t)a.W * a.H + kTexThreads - 1) / kTexThreads), (unsigned)B), block(kTexThreads);
  if (boundary == MR_TEXTURE_WRAP) hipLaunchKernelGGL((k_tex_forward<C, MR_TEXTURE_WRAP>), grid, block, 0, s, a, out);
  else hipLaunchKernelGGL((k_tex_forward<C, MR_TEXTURE_CLAMP>), grid, block, 0, s, a, out);
  return check_launch();
}

template <int C, int MODE>
int launch_backward_c(const TexArgs &a, int B, int boundary, const float *dout, float *dtex,
                      unsigned long long *dtex_fixed, float *duv, DetBlock *det_block, hipStream_t s) {
  const int tiles_x = (a.W + kTileW - 1) / kTileW, tiles_y = (a.H + kTileH - 1) / kTileH;
  const dim3 grid((unsigned)((size_t)tiles_x * tiles_y), (unsigned)B), block(kTexThreads);
  if (boundary == MR_TEXTURE_WRAP)
    hipLaunchKernelGGL((k_tex_backward<C, MR_TEXTURE_WRAP, MODE>), grid, block, 0, s, a, tiles_x, dout, dtex,
                       dtex_fixed, (float2 *)duv, det_block);
  else
    hipLaunchKernelGGL((k_tex_backward<C, MR_TEXTURE_CLAMP, MODE>), grid, block, 0, s, a, tiles_x, dout, dtex,
                       dtex_fixed, (float2 *)duv, det_block);
  return check_launch();
}

template <int MODE>
int launch_backward_mode(const TexArgs &a, int C, int B, int boundary, const float *dout, float *dtex,
                         unsigned long long *dtex_fixed, float *duv, DetBlock *det_block, hipStream_t s) {
  switch (C) {
    case 1: return launch_backward_c<1, MODE>(a, B, boundary, dout, dtex, dtex_fixed, duv, det_block, s);
    case 2: return launch_backward_c<2, MODE>(a, B, boundary, dout, dtex, dtex_fixed, duv, det_block, s);
    case 3: return launch_backward_c<3, MODE>(a, B, boundary, dout, dtex, dtex_fixed, duv, det_block, s);
    default: return launch_backward_c<4, MODE>(a, B, boundary, dout, dtex, dtex_fixed, duv, det_block, s);
  }
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
  switch (C) {
    case 1: return launch_forward_c<1>(a, B, boundary, out, s);
    case 2: return launch_forward_c<2>(a, B, boundary, out, s);
    case 3: return launch_forward_c<3>(a, B, boundary, out, s);
    default: return launch_forward_c<4>(a, B, boundary, out, s);
  }
}

int launch_texture_backward(const float *dout, const float *tex, int tex_batched, int Ht, int Wt, int C,
                            const float *uv, const float *mask, int B, int W, int H, int boundary, float *dtex,
                            float *duv, void *ws, hipStream_t s) {
  if (B == 0 || (!dtex && !duv)) return MR_OK;
  const TexArgs a = make_args(tex, tex_batched, Ht, Wt, C, uv, mask, W, H);
  const size_t n_tex = tex_floats(tex_batched, Ht, Wt, C, B);
  if (!dtex || g_deterministic == 0) {
    if (dtex && zero_async(dtex, n_tex * sizeof(float), s) != hipSuccess) return check_launch();
    return launch_backward_mode<kModeFloat>(a, C, B, boundary, dout, dtex, nullptr, duv, nullptr, s);
  }
  // Deterministic: the scale comes from the largest |dout| (every contribution is w * dout with w <= 1) and the
  // number of pixels that sample one texture, so that no texel's sum can leave the 64-bit range.
  unsigned long long *fixed = (unsigned long long *)ws;
  DetBlock *det_block = (DetBlock *)((char *)ws + fixed_bytes(tex_batched, Ht, Wt, C, B));
  if (zero_async(fixed, fixed_bytes(tex_batched, Ht, Wt, C, B), s) != hipSuccess) return check_launch();
  const double per_texture = (double)(tex_batched ? 1 : B) * W * H;
  const float gain = (float)fmax(1.0, per_texture / (double)(1 << 21));
  int rc = launch_det_scale(dout, (size_t)B * W * H * C, gain, det_block, s);
  if (rc != MR_OK) return rc;
  rc = launch_backward_mode<kModeFixed>(a, C, B, boundary, dout, nullptr, fixed, duv, det_block, s);
  if (rc != MR_OK) return rc;
  return launch_det_to_float((const long long *)fixed, det_block, dtex, n_tex, s);
}

}  // namespace mr
