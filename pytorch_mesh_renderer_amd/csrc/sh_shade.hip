// Second-order spherical-harmonics irradiance shading of a pixel buffer (mr_sh_shade_forward / _backward).
//
// Semantics: INTEGRATION.md, "Spherical-harmonics lighting".  Per pixel: n = N / max(|N|, 1e-12),
// E_c = sum_k sh[b,k,c] Y_k(n) (irradiance coefficients, no clamp), rgb = diffuse * E, rgb = 0 where alpha <= 0.5,
// RGBA out with the rows flipped or not.
//
// Layout: one lane per pixel; a workgroup covers a contiguous run of one image's pixels (grid = (runs, B)), so the
// image's 27 coefficients are wave-uniform and come in through scalar loads.  Normals and diffuse colour are read
// through two pointers with one pixel stride: two [B,H,W,3] buffers (stride 3) or two channel slices of one packed
// [B,H,W,C] buffer (stride C).
//
// The backward is in gather form: each lane writes only its own pixel's dnormals / ddiffuse / dalphas.  The 27 dsh
// sums of an image are accumulated in registers over kShBwdPixels pixels per lane, reduced across the wavefront with
// DPP, across the workgroup's waves through LDS, and written as one row per workgroup to the workspace; a second
// launch sums each image's rows in a fixed order.  No atomics and no memsets: every output is written completely by
// a kernel and dsh is bit-reproducible.  The row count depends on the image size only.
#include "mr_internal.h"

namespace mr {

namespace {

constexpr int kShThreads = 256;       // 4 wavefronts
constexpr int kShBwdPixels = 4;       // pixels per lane in the backward: the dsh reduction is paid once per 4
constexpr int kShTerms = 27;          // 9 basis functions x 3 channels, index 3 k + c
constexpr int kShBwdRun = kShThreads * kShBwdPixels;
constexpr float kShEps = 1e-12f;      // F.normalize's default eps
static_assert(kShThreads == 4 * kWave, "block_sum_terms sums four wavefronts");

constexpr float kY0 = 0.282094791773878f;
constexpr float kY1 = 0.488602511902920f;
constexpr float kY4 = 1.092548430592079f;
constexpr float kY6 = 0.315391565252520f;
constexpr float kY8 = 0.546274215296040f;

__device__ __forceinline__ void sh_basis(float x, float y, float z, float Y[9]) {
  Y[0] = kY0;
  Y[1] = kY1 * y;
  Y[2] = kY1 * z;
  Y[3] = kY1 * x;
  Y[4] = kY4 * x * y;
  Y[5] = kY4 * y * z;
  Y[6] = kY6 * (3.0f * z * z - 1.0f);
  Y[7] = kY4 * x * z;
  Y[8] = kY8 * (x * x - y * y);
}

// the output (and upstream-gradient) pixel of input pixel p of image b
__device__ __forceinline__ size_t out_pixel(int b, int p, int W, int H, int flip) {
  const size_t img = (size_t)b * W * H;
  if (!flip) return img + p;
  const int y = p / W, x = p - y * W;
  return img + (size_t)(H - 1 - y) * W + x;
}

__device__ __forceinline__ float pixel_alpha(const float *__restrict__ alphas, size_t i, float d0, float d1, float d2) {
  if (alphas) return alphas[i];
  return (d0 >= 0.0f || d1 >= 0.0f || d2 >= 0.0f) ? 1.0f : 0.0f;  // render()'s rule: background diffuse is -1
}

__device__ __forceinline__ void load_sh(const float *__restrict__ sh, int b, float c[kShTerms]) {
  const float *s = sh + (size_t)b * kShTerms;  // b = blockIdx.y: wave-uniform, scalar loads
#pragma unroll
  for (int k = 0; k < kShTerms; ++k) c[k] = s[k];
}

// ---- forward ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kShThreads) void k_sh_forward(const float *__restrict__ normals,
                                                           const float *__restrict__ diffuse, int stride,
                                                           const float *__restrict__ alphas,
                                                           const float *__restrict__ sh, int W, int H, int flip,
                                                           float *__restrict__ rgba) {
  const int b = (int)blockIdx.y;
  const int hw = W * H;
  float c[kShTerms];
  load_sh(sh, b, c);
  const int p = (int)blockIdx.x * kShThreads + (int)threadIdx.x;
  if (p >= hw) return;
  const size_t i = (size_t)b * hw + p;
  const float *np = normals + i * stride;
  const float *dp = diffuse + i * stride;
  const float d0 = dp[0], d1 = dp[1], d2 = dp[2];
  const float alpha = pixel_alpha(alphas, i, d0, d1, d2);
  float4 o = make_float4(0.0f, 0.0f, 0.0f, alpha);
  if (alpha > 0.5f) {
    const float nx = np[0], ny = np[1], nz = np[2];
    const float r = fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), kShEps);
    float Y[9];
    sh_basis(nx / r, ny / r, nz / r, Y);
    float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      e0 += c[3 * k + 0] * Y[k];
      e1 += c[3 * k + 1] * Y[k];
      e2 += c[3 * k + 2] * Y[k];
    }
    o.x = d0 * e0;
    o.y = d1 * e1;
    o.z = d2 * e2;
  }
  *(float4 *)(rgba + out_pixel(b, p, W, H, flip) * 4) = o;  // 16-B aligned: checked in abi.hip
}

// ---- backward ---------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// The sum of v over the wavefront, the same on every lane.  Within each 16-lane row: quad_perm [1,0,3,2],
// quad_perm [2,3,0,1], row_half_mirror, row_mirror -- after each step the two partners hold the same (commuted)
// sum, so the row's lanes agree bit for bit; then the four row sums in a fixed order.
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v += dpp_f<0xb1>(v);
  v += dpp_f<0x4e>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
  return (readlane_f(v, 0) + readlane_f(v, 16)) + (readlane_f(v, 32) + readlane_f(v, 48));
}

// The workgroup's sums of acc[0..26], written by threads 0..26 to out[0..26].  Every thread of the workgroup calls it.
__device__ __forceinline__ void block_sum_terms(const float acc[kShTerms], float *__restrict__ out) {
  __shared__ float part[kShThreads / kWave][kShTerms];
  const int wave = (int)threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < kShTerms; ++k) {
    const float s = wave_sum_dpp(acc[k]);
    if (lane_id() == 0) part[wave][k] = s;
  }
  __syncthreads();
  const int t = (int)threadIdx.x;
  if (t < kShTerms) out[t] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
}

__global__ __launch_bounds__(kShThreads) void k_sh_backward(const float *__restrict__ drgba,
                                                            const float *__restrict__ normals,
                                                            const float *__restrict__ diffuse, int stride,
                                                            const float *__restrict__ alphas,
                                                            const float *__restrict__ sh, int W, int H, int flip,
                                                            float *__restrict__ dnormals, float *__restrict__ ddiffuse,
                                                            float *__restrict__ dalphas, float *__restrict__ rows) {
  const int b = (int)blockIdx.y;
  const int hw = W * H;
  float c[kShTerms];
  load_sh(sh, b, c);
  float acc[kShTerms];
#pragma unroll
  for (int k = 0; k < kShTerms; ++k) acc[k] = 0.0f;
  const int first = (int)blockIdx.x * kShBwdRun + (int)threadIdx.x;
  for (int j = 0; j < kShBwdPixels; ++j) {
    const int p = first + j * kShThreads;
    if (p >= hw) break;
    const size_t i = (size_t)b * hw + p;
    const float4 g = *(const float4 *)(drgba + out_pixel(b, p, W, H, flip) * 4);  // 16-B aligned: abi.hip
    if (dalphas) dalphas[i] = g.w;
    const float *dp = diffuse + i * stride;
    const float d0 = dp[0], d1 = dp[1], d2 = dp[2];
    const float alpha = pixel_alpha(alphas, i, d0, d1, d2);
    float *dn = dnormals ? dnormals + i * stride : nullptr;
    float *dd = ddiffuse ? ddiffuse + i * stride : nullptr;
    if (!(alpha > 0.5f)) {  // masked: no gradient to the normal or the colour, nothing to dsh
      if (dn) { dn[0] = 0.0f; dn[1] = 0.0f; dn[2] = 0.0f; }
      if (dd) { dd[0] = 0.0f; dd[1] = 0.0f; dd[2] = 0.0f; }
      continue;
    }
    const float *np = normals + i * stride;
    const float nx = np[0], ny = np[1], nz = np[2];
    const float len = sqrtf(nx * nx + ny * ny + nz * nz);
    const float r = fmaxf(len, kShEps);
    const float x = nx / r, y = ny / r, z = nz / r;
    float Y[9];
    sh_basis(x, y, z, Y);
    // dE_c = g_c d_c;  dsh[k][c] += Y_k dE_c
    const float de0 = g.x * d0, de1 = g.y * d1, de2 = g.z * d2;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      acc[3 * k + 0] += Y[k] * de0;
      acc[3 * k + 1] += Y[k] * de1;
      acc[3 * k + 2] += Y[k] * de2;
    }
    if (dd) {
      float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        e0 += c[3 * k + 0] * Y[k];
        e1 += c[3 * k + 1] * Y[k];
        e2 += c[3 * k + 2] * Y[k];
      }
      dd[0] = g.x * e0;
      dd[1] = g.y * e1;
      dd[2] = g.z * e2;
    }
    if (dn) {
      float dY[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) dY[k] = (c[3 * k + 0] * de0 + c[3 * k + 1] * de1) + c[3 * k + 2] * de2;
      // d/dn of the basis (Y_0 is constant)
      const float gx = kY1 * dY[3] + kY4 * (y * dY[4] + z * dY[7]) + 2.0f * kY8 * x * dY[8];
      const float gy = kY1 * dY[1] + kY4 * (x * dY[4] + z * dY[5]) - 2.0f * kY8 * y * dY[8];
      const float gz = kY1 * dY[2] + kY4 * (y * dY[5] + x * dY[7]) + 6.0f * kY6 * z * dY[6];
      // through n = N / max(|N|, eps): (g - n (n . g)) / |N| while |N| >= eps, g / eps below (F.normalize)
      float ox = gx, oy = gy, oz = gz;
      if (len >= kShEps) {
        const float ng = (x * gx + y * gy) + z * gz;
        ox = gx - x * ng;
        oy = gy - y * ng;
        oz = gz - z * ng;
      }
      dn[0] = ox / r;
      dn[1] = oy / r;
      dn[2] = oz / r;
    }
  }
  if (rows) block_sum_terms(acc, rows + ((size_t)b * gridDim.x + blockIdx.x) * kShTerms);  // rows: uniform
}

// dsh[b] = the sum of image b's `count` workspace rows, in a fixed order (one workgroup per image)
__global__ __launch_bounds__(kShThreads) void k_sh_sum_rows(const float *__restrict__ rows, int count,
                                                            float *__restrict__ dsh) {
  const int b = (int)blockIdx.x;
  float acc[kShTerms];
#pragma unroll
  for (int k = 0; k < kShTerms; ++k) acc[k] = 0.0f;
  const float *img = rows + (size_t)b * count * kShTerms;
  for (int r = (int)threadIdx.x; r < count; r += kShThreads) {
#pragma unroll
    for (int k = 0; k < kShTerms; ++k) acc[k] += img[(size_t)r * kShTerms + k];
  }
  block_sum_terms(acc, dsh + (size_t)b * kShTerms);
}

inline unsigned fwd_runs(int W, int H) { return (unsigned)(((size_t)W * H + kShThreads - 1) / kShThreads); }
inline unsigned bwd_runs(int W, int H) { return (unsigned)(((size_t)W * H + kShBwdRun - 1) / kShBwdRun); }

}  // namespace

size_t sh_shade_backward_ws(int B, int W, int H) {
  return align_up((size_t)B * bwd_runs(W, H) * kShTerms * sizeof(float), 256);
}

int launch_sh_shade_forward(const float *normals, const float *diffuse, int stride, const float *alphas,
                            const float *sh, int B, int W, int H, int flip, float *rgba, hipStream_t s) {
  if (B == 0) return MR_OK;
  hipLaunchKernelGGL(k_sh_forward, dim3(fwd_runs(W, H), (unsigned)B), dim3(kShThreads), 0, s, normals, diffuse,
                     stride, alphas, sh, W, H, flip, rgba);
  return check_launch();
}

int launch_sh_shade_backward(const float *drgba, const float *normals, const float *diffuse, int stride,
                             const float *alphas, const float *sh, int B, int W, int H, int flip, float *dnormals,
                             float *ddiffuse, float *dalphas, float *dsh, void *ws, hipStream_t s) {
  if (B == 0) return MR_OK;
  const unsigned runs = bwd_runs(W, H);
  float *rows = dsh ? (float *)ws : nullptr;
  hipLaunchKernelGGL(k_sh_backward, dim3(runs, (unsigned)B), dim3(kShThreads), 0, s, drgba, normals, diffuse, stride,
                     alphas, sh, W, H, flip, dnormals, ddiffuse, dalphas, rows);
  int rc = check_launch();
  if (rc != MR_OK || !dsh) return rc;
  hipLaunchKernelGGL(k_sh_sum_rows, dim3((unsigned)B), dim3(kShThreads), 0, s, (const float *)rows, (int)runs, dsh);
  return check_launch();
}

}  // namespace mr
