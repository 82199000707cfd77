// Analytic silhouette antialiasing of a rasterized image (mr_antialias_forward / _backward).
//
// Semantics: INTEGRATION.md, "Silhouette antialiasing".  In short: every horizontal and vertical pair of
// neighbouring pixels whose ids differ (or exactly one of which is covered) is looked at once; the front pixel
// f's triangle F is left by the segment f->g through one of its edges at t in [0, 1]; if that edge is a
// silhouette of the mesh, the colours of the two pixels are blended by how far past (or short of) the segment
// midpoint the edge lies, and t is differentiated with respect to the edge's clip-space vertices.  The derivative is
// taken at the crossing point of the DECIDED t, P_c = f + t (g - f) with t clamped and rounded as rule 5 left it: where
// the clamp acted (a G-buffer that does not belong to clip) that is an end of the segment, and the gradient is rule 8's
// formula there -- neither the slope of the unclamped quotient nor zero (tests/antialias_reference.py says the same).
//
// Layout: one lane per pixel, a workgroup is 64 x 4 pixels (one wavefront per row), so that the left / right
// neighbours of a lane come from the wavefront's own lines and the up / down ones from the lines of the
// neighbouring wavefronts.  GATHER form: every lane evaluates the (up to) four pairs it belongs to and writes only
// its own output pixel -- each pair is evaluated by both of its pixels, with the same operations on the same
// operands, so both agree on it bit for bit.  The forward has no atomics.  The backward's image gradient is
// gathered the same way; its clip-space gradient is scattered by the lane of the pair's MODIFIED pixel (exactly
// one per blended pair), summed within the wavefront per vertex first.
//
// Discrete decisions (coverage, front pixel, edge functions, exit edge, silhouette orientation) are binary32,
// un-fused, in the documented order: this file is compiled with -ffp-contract=off (Makefile), so that a float32
// restatement reproduces the set of blended pairs exactly.  The edge functions are those of the rasterizer
// (raster_forward.hip): the sign-normalised adjugate rows of [[x],[y],[w]].
#include "mr_internal.h"
#include "det_fixed.h"

namespace mr {

extern thread_local int g_deterministic;  // mr_set_deterministic (shade.hip)

namespace {

constexpr int kAaW = 64, kAaRows = 4, kAaThreads = kAaW * kAaRows;
constexpr float kCoveredBary = 0.9f;  // the reference's skip rule (rasterize_triangles.cpp:162)

struct AaArgs {
  const float *image;  // [B,H,W,C]
  const int32_t *ids;  // [B,H,W]
  const float *bary;   // [B,H,W,3]
  const float *z;      // [B,H,W]
  const float *clip;   // [B,V,4]
  const int32_t *tris;  // [T,3]
  const int32_t *opp;   // [T,3]: neighbour's opposite vertex across the edge opposite corner k; -1 / -2
  int B, V, T, W, H, C;
  float hw, hh;  // (float)(0.5 * W), (float)(0.5 * H)
};

// what a pixel contributes to a pair decision
struct Px {
  int ix, iy, id;
  bool cov;
  float cx, cy;  // NDC pixel centre (with_centres)
};

__device__ __forceinline__ float centre_x(int ix, float hw) { return (float)(((double)ix + 0.5) / (double)hw - 1.0); }
__device__ __forceinline__ float centre_y(int iy, float hh) { return (float)(((double)iy + 0.5) / (double)hh - 1.0); }

__device__ __forceinline__ bool covered(const AaArgs &a, size_t pix, int id) {
  if (id != 0) return true;
  const float *b = a.bary + pix * 3;
  return (b[0] + b[1]) + b[2] >= kCoveredBary;
}

// The outcome of one pair.  blend: the pair changes a pixel; mod_f: that pixel is f (t < 0.5) rather than g.
struct Pair {
  bool blend, mod_f, f_is_p;
  float t;
  int va, vb;                 // exit edge's vertices (corners k+1, k+2 of F)
  float ax, ay, aw, bx, by, bw;  // their clip x, y, w
  float pcx, pcy;             // the crossing point in NDC
  float inv_d;                // s / (e(f) - e(g)), s = the adjugate's sign, from the exact centre difference
};

// p: the lane's pixel, q: its neighbour (horizontal: dy == 0).  Both lanes of a pair run this with the roles of p
// and q swapped; every decision below is symmetric in the two (f / g are chosen from the pixels' data only).
__device__ Pair eval_pair(const AaArgs &a, int b, const Px &p, const Px &q, size_t pix_p, size_t pix_q,
                          bool horizontal) {
  Pair r;
  r.blend = false;
  if (p.id == q.id && p.cov == q.cov) return r;
  bool f_is_p;
  if (p.cov != q.cov) {
    f_is_p = p.cov;
  } else {
    const float zp = a.z[pix_p], zq = a.z[pix_q];
    f_is_p = zp < zq || (zp == zq && p.id > q.id);
  }
  r.f_is_p = f_is_p;
  const Px &f = f_is_p ? p : q;
  const Px &g = f_is_p ? q : p;
  const int F = f.id;
  if ((unsigned)F >= (unsigned)a.T) return r;
  int vi[3];
  for (int k = 0; k < 3; ++k) {
    vi[k] = a.tris[3 * F + k];
    if ((unsigned)vi[k] >= (unsigned)a.V) return r;
  }
  const float *cb = a.clip + (size_t)b * a.V * 4;
  float x[3], y[3], w[3];
  for (int k = 0; k < 3; ++k) {
    const float4 v = *(const float4 *)(cb + (size_t)vi[k] * 4);
    x[k] = v.x; y[k] = v.y; w[k] = v.w;
  }
  if (w[0] <= 0.0f || w[1] <= 0.0f || w[2] <= 0.0f) return r;
  // adjugate of [[x0 x1 x2] [y0 y1 y2] [w0 w1 w2]], sign-normalised: SURVEY.md Appendix A, as raster_forward.hip
  const float a11 = x[0], a12 = x[1], a13 = x[2], a21 = y[0], a22 = y[1], a23 = y[2], a31 = w[0], a32 = w[1], a33 = w[2];
  float m[9];
  m[0] = a22 * a33 - a32 * a23; m[1] = a13 * a32 - a33 * a12; m[2] = a12 * a23 - a22 * a13;
  m[3] = a23 * a31 - a33 * a21; m[4] = a11 * a33 - a31 * a13; m[5] = a13 * a21 - a23 * a11;
  m[6] = a21 * a32 - a31 * a22; m[7] = a12 * a31 - a32 * a11; m[8] = a11 * a22 - a21 * a12;
  const float det = (a11 * m[0] + a12 * m[3]) + a13 * m[6];
  if (det < 0.0f) {
    for (int k = 0; k < 9; ++k) m[k] = -m[k];
  }
  const float fx = f.cx, fy = f.cy, gx = g.cx, gy = g.cy;
  int exit = -1;
  float t = 0.0f;
  for (int k = 0; k < 3; ++k) {
    const float ef = (m[3 * k] * fx + m[3 * k + 1] * fy) + m[3 * k + 2];
    const float eg = (m[3 * k] * gx + m[3 * k + 1] * gy) + m[3 * k + 2];
    if (!(eg < 0.0f)) continue;
    float tk = ef / (ef - eg);
    tk = fminf(fmaxf(tk, 0.0f), 1.0f);
    if (exit < 0 || tk < t) {
      exit = k;
      t = tk;
    }
  }
  if (exit < 0) return r;
  const int ka = exit == 2 ? 0 : exit + 1, kb = exit == 0 ? 2 : exit - 1;
  // silhouette: boundary / non-manifold edge, a neighbour behind the camera plane, or the neighbour's far vertex d
  // on the same side of the edge's line as F's own third corner c (zero counts as the same side)
  const int d = a.opp[3 * F + exit];
  if (d >= 0) {
    if (d >= a.V) return r;
    const float4 vd = *(const float4 *)(cb + (size_t)d * 4);
    if (vd.w > 0.0f) {
      const float sc = (m[3 * exit] * x[exit] + m[3 * exit + 1] * y[exit]) + m[3 * exit + 2] * w[exit];
      const float sd = (m[3 * exit] * vd.x + m[3 * exit + 1] * vd.y) + m[3 * exit + 2] * vd.w;
      if ((sc > 0.0f && sd < 0.0f) || (sc < 0.0f && sd > 0.0f)) return r;  // the surface continues: interior edge
    }
  }
  if (t == 0.5f) return r;
  r.blend = true;
  r.mod_f = t < 0.5f;
  r.t = t;
  r.va = vi[ka]; r.vb = vi[kb];
  r.ax = x[ka]; r.ay = y[ka]; r.aw = w[ka];
  r.bx = x[kb]; r.by = y[kb]; r.bw = w[kb];
  r.pcx = fx + t * (gx - fx);
  r.pcy = fy + t * (gy - fy);
  // e(f) - e(g) = m_row . (P_f - P_g): one component of the difference is zero, the constant term cancels.
  // The row is the adjugate's sign times v_a x v_b: that sign goes with the derivative of the cross product.
  r.inv_d = (det < 0.0f ? -1.0f : 1.0f) / (horizontal ? m[3 * exit] * (fx - gx) : m[3 * exit + 1] * (fy - gy));
  return r;
}

__device__ __forceinline__ bool modifies_p(const Pair &r) { return r.blend && (r.mod_f == r.f_is_p); }

// weight of the OTHER pixel's colour in the modified pixel: (t - 0.5) when g is modified, (0.5 - t) when f is
__device__ __forceinline__ float pair_weight(const Pair &r) { return r.mod_f ? 0.5f - r.t : r.t - 0.5f; }

// The lane's pixel and its (up to) four neighbours, in the fixed order left, right, down, up (rows: row 0 is the
// bottom scanline, "down" is iy - 1).
struct Hood {
  bool valid;
  int b;
  Px p, n[4];
  bool has[4];
  size_t pix, npix[4];
  bool uniform;  // every neighbour has p's id and coverage: nothing to do
};

__device__ __forceinline__ Hood load_hood(const AaArgs &a, int block) {
  Hood h;
  const int tiles_x = (a.W + kAaW - 1) / kAaW, tiles_y = (a.H + kAaRows - 1) / kAaRows;
  const int per_image = tiles_x * tiles_y;
  h.b = block / per_image;
  const int r = block - h.b * per_image;
  const int ty = r / tiles_x, tx = r - ty * tiles_x;
  const int ix = tx * kAaW + (int)(threadIdx.x & (kAaW - 1));
  const int iy = ty * kAaRows + (int)(threadIdx.x / kAaW);
  h.valid = h.b < a.B && ix < a.W && iy < a.H;
  h.uniform = true;
  if (!h.valid) return h;
  const size_t img = (size_t)h.b * a.H * a.W;
  h.pix = img + (size_t)iy * a.W + ix;
  h.p.ix = ix; h.p.iy = iy;
  h.p.id = a.ids[h.pix];
  h.p.cov = covered(a, h.pix, h.p.id);
  const int dx[4] = {-1, 1, 0, 0}, dy[4] = {0, 0, -1, 1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int jx = ix + dx[k], jy = iy + dy[k];
    h.has[k] = jx >= 0 && jx < a.W && jy >= 0 && jy < a.H;
    if (!h.has[k]) continue;
    h.npix[k] = img + (size_t)jy * a.W + jx;
    h.n[k].ix = jx; h.n[k].iy = jy;
    h.n[k].id = a.ids[h.npix[k]];
    h.n[k].cov = covered(a, h.npix[k], h.n[k].id);
    h.uniform = h.uniform && h.n[k].id == h.p.id && h.n[k].cov == h.p.cov;
  }
  return h;
}

// The NDC centres of the lane's pixel and its neighbours: six binary64 divisions per lane instead of four per pair.
__device__ __forceinline__ void with_centres(const AaArgs &a, Hood &h) {
  h.p.cx = centre_x(h.p.ix, a.hw);
  h.p.cy = centre_y(h.p.iy, a.hh);
  h.n[0].cx = centre_x(h.p.ix - 1, a.hw); h.n[0].cy = h.p.cy;
  h.n[1].cx = centre_x(h.p.ix + 1, a.hw); h.n[1].cy = h.p.cy;
  h.n[2].cx = h.p.cx; h.n[2].cy = centre_y(h.p.iy - 1, a.hh);
  h.n[3].cx = h.p.cx; h.n[3].cy = centre_y(h.p.iy + 1, a.hh);
}

template <int C>
__device__ __forceinline__ int channels(const AaArgs &a) { return C > 0 ? C : a.C; }

// ---- forward ----------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(kAaThreads) void k_aa_forward(AaArgs a, float *__restrict__ out, uint8_t *__restrict__ pair_mask) {
  Hood h = load_hood(a, (int)blockIdx.x);
  if (!h.valid) return;
  const int nc = channels<C>(a);
  const float *cp = a.image + h.pix * nc;
  float *op = out + h.pix * nc;
  if (h.uniform) {
    if (C == 4) {
      *(float4 *)op = *(const float4 *)cp;  // 16-B aligned: the image is contiguous [.., 4] f32
    } else {
      for (int c = 0; c < nc; ++c) op[c] = cp[c];
    }
    if (pair_mask) pair_mask[h.pix] = 0;
    return;
  }
  with_centres(a, h);
  Pair pr[4];
  unsigned mask = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    pr[k].blend = false;
    if (h.has[k]) pr[k] = eval_pair(a, h.b, h.p, h.n[k], h.pix, h.npix[k], k < 2);
    if (modifies_p(pr[k])) mask |= 1u << k;
  }
  if (pair_mask) pair_mask[h.pix] = (uint8_t)mask;
  // out[p] = c_p + sum over the pairs that modify p, in the order left, right, down, up, of
  //   (t - 0.5) * (c_f - c_g)   when p = g,      (0.5 - t) * (c_g - c_f)   when p = f
  // (both are weight * (c_other - c_p)).
  for (int c = 0; c < nc; ++c) {
    const float own = cp[c];
    float v = own;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(mask & (1u << k))) continue;
      const float other = a.image[h.npix[k] * nc + c];
      v = v + pair_weight(pr[k]) * (other - own);
    }
    op[c] = v;
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------
// MODE: 0 = float atomics into dclip; 1 = only the largest |contribution| (deterministic mode's scale, no dimage);
// 2 = 64-bit fixed point into the workspace (deterministic mode)
constexpr int kModeFloat = 0, kModeMax = 1, kModeFixed = 2;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);  // fixed butterfly: the same sum on every lane
  return v;
}

template <int C, int MODE>
__global__ __launch_bounds__(kAaThreads) void k_aa_backward(AaArgs a, const float *__restrict__ dout,
                                                            float *__restrict__ dimage, float *__restrict__ dclip,
                                                            long long *__restrict__ dclip_fixed,
                                                            DetBlock *__restrict__ det_block) {
  Hood h = load_hood(a, (int)blockIdx.x);
  const int nc = channels<C>(a);
  // up to four pairs where this lane's pixel is the modified one, two vertices each: (vertex, dL/d(x, y, w))
  int key[8];
  float gx[8], gy[8], gw[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    key[s] = -1;
    gx[s] = gy[s] = gw[s] = 0.0f;
  }
  if (h.valid) {
    const float *cp = a.image + h.pix * nc;
    const float *dp = dout + h.pix * nc;
    if (h.uniform) {
      if (MODE != kModeMax) {
        float *op = dimage + h.pix * nc;
        if (C == 4) {
          *(float4 *)op = *(const float4 *)dp;
        } else {
          for (int c = 0; c < nc; ++c) op[c] = dp[c];
        }
      }
    } else {
      with_centres(a, h);
      Pair pr[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        pr[k].blend = false;
        if (h.has[k]) pr[k] = eval_pair(a, h.b, h.p, h.n[k], h.pix, h.npix[k], k < 2);
      }
      // image: out[m] = c_m + w (c_o - c_m)  ->  dc_m += dout[m] (1 - w),  dc_o += dout[m] w
      if (MODE != kModeMax) {
        for (int c = 0; c < nc; ++c) {
          const float own = dp[c];
          float v = own;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (!pr[k].blend) continue;
            if (pr[k].mod_f == pr[k].f_is_p) v = v - pair_weight(pr[k]) * own;
            else v = v + pair_weight(pr[k]) * dout[h.npix[k] * nc + c];
          }
          dimage[h.pix * nc + c] = v;
        }
      }
      // clip: dL/dt = sum_ch dout[m] (c_f - c_g) on either side of 0.5;  dt/dv_a = s (v_b x P_c) / D,
      // dt/dv_b = s (P_c x v_a) / D with P_c = (x, y, 1) the crossing point, D = e(f) - e(g)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!modifies_p(pr[k])) continue;
        const float *cq = a.image + h.npix[k] * nc;
        float dldt = 0.0f;
        for (int c = 0; c < nc; ++c) {
          const float cf = pr[k].f_is_p ? cp[c] : cq[c], cg = pr[k].f_is_p ? cq[c] : cp[c];
          dldt += dp[c] * (cf - cg);
        }
        const Pair &r = pr[k];
        const float s = dldt * r.inv_d;
        const float px = r.pcx, py = r.pcy;
        // v_b x P_c with v = (x, y, w), P = (px, py, 1)
        key[2 * k] = h.b * a.V + r.va;
        gx[2 * k] = s * (r.by * 1.0f - r.bw * py);
        gy[2 * k] = s * (r.bw * px - r.bx * 1.0f);
        gw[2 * k] = s * (r.bx * py - r.by * px);
        // P_c x v_a
        key[2 * k + 1] = h.b * a.V + r.vb;
        gx[2 * k + 1] = s * (py * r.aw - 1.0f * r.ay);
        gy[2 * k + 1] = s * (1.0f * r.ax - px * r.aw);
        gw[2 * k + 1] = s * (px * r.ay - py * r.ax);
      }
    }
  }
  // wave-uniform from here on: every lane, in range or not, takes part in the per-vertex reduction
  bool mine = false;
#pragma unroll
  for (int s = 0; s < 8; ++s) mine |= key[s] >= 0;
  unsigned long long pending = __ballot(mine);
  while (pending) {
    const int leader = __ffsll((long long)pending) - 1;
    int first = -1;
#pragma unroll
    for (int s = 7; s >= 0; --s) first = key[s] >= 0 ? key[s] : first;
    const int K = __builtin_amdgcn_readlane(first, leader);
    float sx = 0.0f, sy = 0.0f, sw = 0.0f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (key[s] == K) {
        sx += gx[s]; sy += gy[s]; sw += gw[s];
        key[s] = -1;
      }
    }
    sx = wave_sum(sx); sy = wave_sum(sy); sw = wave_sum(sw);
    if (lane_id() == leader) {
      if (MODE == kModeFloat) {
        float *dst = dclip + (size_t)K * 4;
        atomicAdd(dst + 0, sx);
        atomicAdd(dst + 1, sy);
        atomicAdd(dst + 3, sw);  // the z column never receives gradient
      } else if (MODE == kModeMax) {
        const float big = fmaxf(fmaxf(fabsf(sx), fabsf(sy)), fabsf(sw));
        atomicMax(&det_block->max_bits, __float_as_int(big != big ? INFINITY : big));
      } else {
        long long *dst = dclip_fixed + (size_t)K * 4;
        const float to_fixed = det_block->to_fixed;
        int *overflow = &det_block->overflow;
        atomic_add_fixed(dst + 0, sx, to_fixed, overflow);
        atomic_add_fixed(dst + 1, sy, to_fixed, overflow);
        atomic_add_fixed(dst + 3, sw, to_fixed, overflow);
      }
    }
    mine = false;
#pragma unroll
    for (int s = 0; s < 8; ++s) mine |= key[s] >= 0;
    pending = __ballot(mine);
  }
}

AaArgs make_args(const float *image, const int32_t *ids, const float *bary, const float *z, const float *clip,
                 const int32_t *tris, const int32_t *opp, int B, int V, int T, int W, int H, int C) {
  AaArgs a{image, ids, bary, z, clip, tris, opp, B, V, T, W, H, C, (float)(0.5 * W), (float)(0.5 * H)};
  return a;
}

unsigned aa_blocks(int B, int W, int H) {
  return (unsigned)((size_t)B * ((W + kAaW - 1) / kAaW) * ((H + kAaRows - 1) / kAaRows));
}

inline size_t fixed_bytes(int B, int V) { return align_up((size_t)B * V * 4 * sizeof(long long), 256); }

template <int MODE>
int launch_backward_mode(const AaArgs &a, const float *dout, float *dimage, float *dclip, long long *fixed,
                         DetBlock *det_block, hipStream_t s) {
  const dim3 grid(aa_blocks(a.B, a.W, a.H)), block(kAaThreads);
  switch (a.C) {
    case 1: hipLaunchKernelGGL((k_aa_backward<1, MODE>), grid, block, 0, s, a, dout, dimage, dclip, fixed, det_block); break;
    case 3: hipLaunchKernelGGL((k_aa_backward<3, MODE>), grid, block, 0, s, a, dout, dimage, dclip, fixed, det_block); break;
    case 4: hipLaunchKernelGGL((k_aa_backward<4, MODE>), grid, block, 0, s, a, dout, dimage, dclip, fixed, det_block); break;
    default: hipLaunchKernelGGL((k_aa_backward<0, MODE>), grid, block, 0, s, a, dout, dimage, dclip, fixed, det_block); break;
  }
  return check_launch();
}

}  // namespace

size_t antialias_backward_ws(int B, int V) { return fixed_bytes(B, V) + kDetBlockBytes; }

int launch_antialias_forward(const float *image, const int32_t *ids, const float *bary, const float *z,
                             const float *clip, const int32_t *tris, const int32_t *opp, int B, int V, int T, int W,
                             int H, int C, float *out, uint8_t *pair_mask, hipStream_t s) {
  if (B == 0) return MR_OK;
  const AaArgs a = make_args(image, ids, bary, z, clip, tris, opp, B, V, T, W, H, C);
  const dim3 grid(aa_blocks(B, W, H)), block(kAaThreads);
  switch (C) {
    case 1: hipLaunchKernelGGL(k_aa_forward<1>, grid, block, 0, s, a, out, pair_mask); break;
    case 3: hipLaunchKernelGGL(k_aa_forward<3>, grid, block, 0, s, a, out, pair_mask); break;
    case 4: hipLaunchKernelGGL(k_aa_forward<4>, grid, block, 0, s, a, out, pair_mask); break;
    default: hipLaunchKernelGGL(k_aa_forward<0>, grid, block, 0, s, a, out, pair_mask); break;
  }
  return check_launch();
}

int launch_antialias_backward(const float *dout, const float *image, const int32_t *ids, const float *bary,
                              const float *z, const float *clip, const int32_t *tris, const int32_t *opp, int B,
                              int V, int T, int W, int H, int C, float *dimage, float *dclip, void *ws,
                              hipStream_t s) {
  if (B == 0) return MR_OK;
  if (V > 0 && zero_async(dclip, (size_t)B * V * 4 * sizeof(float), s) != hipSuccess) return check_launch();
  const AaArgs a = make_args(image, ids, bary, z, clip, tris, opp, B, V, T, W, H, C);
  if (g_deterministic == 0) return launch_backward_mode<kModeFloat>(a, dout, dimage, dclip, nullptr, nullptr, s);
  long long *fixed = (long long *)ws;
  DetBlock *det_block = (DetBlock *)((char *)ws + fixed_bytes(B, V));
  if (zero_async(ws, fixed_bytes(B, V) + kDetBlockBytes, s) != hipSuccess) return check_launch();
  int rc = launch_backward_mode<kModeMax>(a, dout, dimage, dclip, fixed, det_block, s);
  if (rc != MR_OK) return rc;
  if ((rc = launch_det_scale_of_max(det_block, 1.0f, s)) != MR_OK) return rc;
  if ((rc = launch_backward_mode<kModeFixed>(a, dout, dimage, dclip, fixed, det_block, s)) != MR_OK) return rc;
  return launch_det_to_float(fixed, det_block, dclip, (size_t)B * V * 4, s);
}

}  // namespace mr
