// Rigid and similarity registration of matched point sets (mr_align_*; INTEGRATION.md, "Registration").
//
// Row-vector convention s X R + T ~ Y.  The definition is part of the interface (include/mesh_raster.h): weighted
// means, the covariance C = sum w (x - xm)(y - ym)^T / W = U S V^T, R = U E V^T with E = diag(1, 1, det(U V^T))
// (E = I with allow_reflection), s = tr(S E) / var(x), T = ym - s xm R.
//
//   k_align_moments  grid (chunks, B): a workgroup sums eighteen float64 moments over ITS kMomentRows rows of an image
//                    -- W, sum w x, sum w y, sum w x y^T, sum w |x|^2, sum w |y|^2, of x and y minus a reference
//                    point, the chunk's own first kept row of positive weight and its match, so that a cloud far from
//                    the origin loses nothing to cancellation and a row that is not counted (weight 0, dropped,
//                    padded) influences nothing -- and leaves one partial: W, the chunk's means, and the moments
//                    centred on them.  y is read row by row or through an idx plane; a row with idx < 0 (or >= M when
//                    gathering) or with sqdist above the cut-off is dropped.
//   k_align_solve    grid (B): merges an image's partials in a fixed order (eight interleaved groups of chunks, then
//                    the groups in ascending order; the means first, then the moments moved onto them), then ONE lane
//                    does the rest in float64: a one-sided cyclic Jacobi SVD of the 3x3 covariance with a fixed sweep
//                    bound, the determinant correction, scale, translation and the residual in closed form, rounds
//                    once to float32, and keeps ICP's convergence bookkeeping.  A converged image's state is left
//                    untouched.
//   k_align_apply    Xt = s X R + T, padded rows 0.
//   k_align_closest  the closest point sum bary corner of mr_nearest_triangle_forward's (face, bary).
//   k_align_init     ICP's state before the first round (a kernel, not a memset: see zero_async).
//
// A chunk is kMomentRows rows whatever N is, a thread's rows within it and every order of summation are fixed, and a
// chunk beyond an image's length contributes exact zeros: the moments of an image do not depend on the padding of its
// batch, which is what lets a batched ICP equal the single-image calls bit for bit.  No atomics anywhere.
#include <math.h>

#include "mr_internal.h"

namespace mr {
namespace {

constexpr int kMomentThreads = 256;
constexpr int kMomentWaves = kMomentThreads / kWave;
constexpr int kRowsPerThread = 4;
constexpr int kMomentRows = kMomentThreads * kRowsPerThread;   // rows of a chunk
constexpr int kMoments = 18;
constexpr int kMeanSums = 7;       // W and the six first moments
constexpr int kCentredSums = 11;   // the nine cross moments and the two variances
constexpr int kNoRow = 0x7fffffff;
constexpr int kSolveThreads = 256;
constexpr int kSolveWaves = kSolveThreads / kWave;
constexpr int kSolveGroups = kSolveThreads / 32;   // 8 groups of 32 lanes, lane m of a group owns sum m
constexpr int kJacobiSweeps = 16;
constexpr double kRankTolerance = 1e-13;   // a singular value below this multiple of the largest counts as 0

inline int chunks_of(int N) { return (N + kMomentRows - 1) / kMomentRows; }

__device__ __forceinline__ int valid_rows(const int32_t *__restrict__ lengths, int b, int N) {
  return lengths ? min(max(lengths[b], 0), N) : N;
}

// grid (chunks, B).  partials [B][chunks][18]: W, the chunk's weighted means of x and of y (3 + 3; 0 where W = 0), and
// eleven moments CENTRED on those means: sum w (x - mx)(y - my)^T (9), sum w |x - mx|^2, sum w |y - my|^2.
__global__ __launch_bounds__(kMomentThreads) void k_align_moments(
    const float *__restrict__ x, const float *__restrict__ y, const int32_t *__restrict__ idx, int gather,
    const float *__restrict__ weights, const float *__restrict__ sqdist, float max_sqdist,
    const int32_t *__restrict__ lengths, const int32_t *__restrict__ converged, int N, int M,
    double *__restrict__ partials) {
  __shared__ double lds[kMomentWaves][kMoments];
  __shared__ double sums[kMoments];
  __shared__ int first_of_wave[kMomentWaves];
  __shared__ float reference[6];
  const int b = (int)blockIdx.y, chunk = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (converged && converged[b]) return;   // (the whole workgroup) a frozen image: nobody reads its partials
  const int nv = valid_rows(lengths, b, N);
  const float *xb = x + (size_t)b * N * 3;
  const float *yb = y + (size_t)b * (gather ? M : N) * 3;
  const int lane = tid & (kWave - 1), wave = tid >> 6;

  // a thread's four rows, loaded once: a dropped row has weight 0 and coordinates 0
  float px[kRowsPerThread][3], py[kRowsPerThread][3];
  double w[kRowsPerThread];
  int first = kNoRow;   // the lowest kept row of positive weight
#pragma unroll
  for (int j = 0; j < kRowsPerThread; ++j) {
    const int i = chunk * kMomentRows + j * kMomentThreads + tid;   // (chunks * kMomentRows < 2^31: N <= 2^28)
    bool kept = i < nv;
    const size_t at = (size_t)b * N + (kept ? i : 0);
    int row = i;
    if (kept && idx) {
      const int k = idx[at];
      if (k < 0 || (gather && k >= M)) kept = false;
      else if (gather) row = k;
    }
    if (kept && sqdist && !(sqdist[at] <= max_sqdist)) kept = false;
    w[j] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) px[j][k] = 0.0f, py[j][k] = 0.0f;
    if (kept) {
      w[j] = weights ? (double)weights[at] : 1.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) px[j][k] = xb[3 * (size_t)i + k], py[j][k] = yb[3 * (size_t)row + k];
      if (w[j] > 0.0 && first == kNoRow) first = j * kMomentThreads + tid;
    }
  }
  // the chunk's reference point: its first kept row of positive weight (0 without one), found by a minimum, handed
  // round through LDS by the thread that holds it.  A row that is not counted never becomes the reference.
  int lowest = first;
#pragma unroll
  for (int step = kWave / 2; step > 0; step >>= 1) lowest = min(lowest, __shfl_xor(lowest, step, kWave));
  if (lane == 0) first_of_wave[wave] = lowest;
  __syncthreads();
  lowest = first_of_wave[0];
#pragma unroll
  for (int wv = 1; wv < kMomentWaves; ++wv) lowest = min(lowest, first_of_wave[wv]);
  if (lowest != kNoRow && (lowest & (kMomentThreads - 1)) == tid) {
    const int mine = lowest / kMomentThreads;
#pragma unroll
    for (int j = 0; j < kRowsPerThread; ++j)
      if (j == mine) {
#pragma unroll
        for (int k = 0; k < 3; ++k) reference[k] = px[j][k], reference[3 + k] = py[j][k];
      }
  }
  __syncthreads();
  double rx[3], ry[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    rx[k] = lowest != kNoRow ? (double)reference[k] : 0.0;
    ry[k] = lowest != kNoRow ? (double)reference[3 + k] : 0.0;
  }

  double acc[kMoments];
#pragma unroll
  for (int m = 0; m < kMoments; ++m) acc[m] = 0.0;
#pragma unroll
  for (int j = 0; j < kRowsPerThread; ++j) {
    const double wj = w[j];
    const double ax = (double)px[j][0] - rx[0], ay = (double)px[j][1] - rx[1], az = (double)px[j][2] - rx[2];
    const double bx = (double)py[j][0] - ry[0], by = (double)py[j][1] - ry[1], bz = (double)py[j][2] - ry[2];
    const double wax = wj * ax, way = wj * ay, waz = wj * az;
    acc[0] += wj;
    acc[1] += wax, acc[2] += way, acc[3] += waz;
    acc[4] += wj * bx, acc[5] += wj * by, acc[6] += wj * bz;
    acc[7] += wax * bx, acc[8] += wax * by, acc[9] += wax * bz;
    acc[10] += way * bx, acc[11] += way * by, acc[12] += way * bz;
    acc[13] += waz * bx, acc[14] += waz * by, acc[15] += waz * bz;
    acc[16] += wax * ax + way * ay + waz * az;
    acc[17] += wj * (bx * bx + by * by + bz * bz);
  }
  // the wavefront's sum in a fixed tree, then the wavefronts in ascending order
#pragma unroll
  for (int m = 0; m < kMoments; ++m) {
    double v = acc[m];
#pragma unroll
    for (int step = kWave / 2; step > 0; step >>= 1) v += __shfl_down(v, step, kWave);
    acc[m] = v;
  }
  if (lane == 0) {
#pragma unroll
    for (int m = 0; m < kMoments; ++m) lds[wave][m] = acc[m];
  }
  __syncthreads();
  if (tid < kMoments) {
    double v = lds[0][tid];
#pragma unroll
    for (int wv = 1; wv < kMomentWaves; ++wv) v += lds[wv][tid];
    sums[tid] = v;
  }
  __syncthreads();
  // from the moments about the reference to the chunk's means and the moments about THEM
  if (tid < kMoments) {
    const double W = sums[0];
    const bool some = W != 0.0;   // (NaN included: it has to reach the solve)
    const double iw = some ? 1.0 / W : 0.0;
    double v = sums[tid];
    if (tid >= 1 && tid < 4) v = some ? rx[tid - 1] + v * iw : 0.0;
    else if (tid >= 4 && tid < 7) v = some ? ry[tid - 4] + v * iw : 0.0;
    else if (tid >= 7 && tid < 16) v -= sums[1 + (tid - 7) / 3] * (sums[4 + (tid - 7) % 3] * iw);
    else if (tid == 16) v -= (sums[1] * sums[1] + sums[2] * sums[2] + sums[3] * sums[3]) * iw;
    else if (tid == 17) v -= (sums[4] * sums[4] + sums[5] * sums[5] + sums[6] * sums[6]) * iw;
    partials[((size_t)b * gridDim.x + chunk) * kMoments + tid] = v;
  }
}

struct Vec3 {
  double x, y, z;
};
__device__ __forceinline__ double dot(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ Vec3 cross(Vec3 a, Vec3 b) {
  return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ Vec3 scaled(Vec3 a, double k) { return Vec3{a.x * k, a.y * k, a.z * k}; }
__device__ __forceinline__ Vec3 minus(Vec3 a, Vec3 b) { return Vec3{a.x - b.x, a.y - b.y, a.z - b.z}; }

// One rotation of the one-sided Jacobi: makes columns p and q of A orthogonal, V follows.
__device__ __forceinline__ bool jacobi_pair(Vec3 &ap, Vec3 &aq, Vec3 &vp, Vec3 &vq) {
  const double alpha = dot(ap, ap), beta = dot(aq, aq), gamma = dot(ap, aq);
  if (!(fabs(gamma) > 1e-16 * sqrt(alpha * beta))) return false;   // orthogonal already (or a zero column)
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  const Vec3 np = minus(scaled(ap, c), scaled(aq, s)), nq{s * ap.x + c * aq.x, s * ap.y + c * aq.y, s * ap.z + c * aq.z};
  const Vec3 wp = minus(scaled(vp, c), scaled(vq, s)), wq{s * vp.x + c * vq.x, s * vp.y + c * vq.y, s * vp.z + c * vq.z};
  ap = np, aq = nq, vp = wp, vq = wq;
  return true;
}

__device__ __forceinline__ void swap_columns(Vec3 &a, Vec3 &b, Vec3 &va, Vec3 &vb, double &sa, double &sb) {
  const Vec3 ta = a, tv = va;
  const double ts = sa;
  a = b, va = vb, sa = sb;
  b = ta, vb = tv, sb = ts;
}

// A unit vector orthogonal to the unit vector u: the axis least aligned with it, made orthogonal.
__device__ __forceinline__ Vec3 any_orthogonal(Vec3 u) {
  const double ax = fabs(u.x), ay = fabs(u.y), az = fabs(u.z);
  const Vec3 e = ax <= ay && ax <= az ? Vec3{1.0, 0.0, 0.0} : (ay <= az ? Vec3{0.0, 1.0, 0.0} : Vec3{0.0, 0.0, 1.0});
  const Vec3 r = minus(e, scaled(u, dot(e, u)));
  return scaled(r, 1.0 / sqrt(dot(r, r)));
}

struct Solution {
  double R[9], T[3], s, mse;
};

// c: the covariance, row-major (c[3 i + j] pairs x_i with y_j).  -> R (row-major) and tr(S E).
__device__ void rotation_of(const double *c, bool allow_reflection, double *R, double *trace) {
  double scale = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) scale = fmax(scale, fabs(c[k]));
  Vec3 v0{1.0, 0.0, 0.0}, v1{0.0, 1.0, 0.0}, v2{0.0, 0.0, 1.0};
  if (!(scale > 0.0)) {   // C = 0: R = I
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    *trace = 0.0;
    return;
  }
  const double inv = 1.0 / scale;
  Vec3 a0{c[0] * inv, c[3] * inv, c[6] * inv}, a1{c[1] * inv, c[4] * inv, c[7] * inv},
      a2{c[2] * inv, c[5] * inv, c[8] * inv};   // the columns of C / scale
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    bool moved = jacobi_pair(a0, a1, v0, v1);
    moved |= jacobi_pair(a0, a2, v0, v2);
    moved |= jacobi_pair(a1, a2, v1, v2);
    if (!moved) break;
  }
  double s0 = sqrt(dot(a0, a0)), s1 = sqrt(dot(a1, a1)), s2 = sqrt(dot(a2, a2));
  if (s0 < s1) swap_columns(a0, a1, v0, v1, s0, s1);
  if (s0 < s2) swap_columns(a0, a2, v0, v2, s0, s2);
  if (s1 < s2) swap_columns(a1, a2, v1, v2, s1, s2);
  // U: u0 from the largest column (scale > 0: s0 > 0); u1 made orthogonal to it, or any orthogonal direction where the
  // covariance has rank 1; the third direction is +-n with n = u0 x u1, never taken from a (possibly zero) column
  const Vec3 u0 = scaled(a0, 1.0 / s0);
  Vec3 u1;
  if (s1 > kRankTolerance * s0) {
    const Vec3 r = minus(a1, scaled(u0, dot(a1, u0)));
    u1 = scaled(r, 1.0 / sqrt(dot(r, r)));
  } else {
    u1 = any_orthogonal(u0);
    s1 = 0.0;
  }
  const Vec3 n = cross(u0, u1);
  const double third = s2 > kRankTolerance * s0 ? dot(a2, n) : 0.0;   // det(U) s2
  const double det_v = dot(v0, cross(v1, v2));                        // +-1
  // without reflection  E_33 u2 = det(U) det(V) u2 = det(V) n  whatever the sign of u2 is
  const double e = allow_reflection ? (third >= 0.0 ? 1.0 : -1.0) : (det_v >= 0.0 ? 1.0 : -1.0);
  const double last = allow_reflection ? fabs(third) : (det_v >= 0.0 ? third : -third);
  *trace = (s0 + s1 + last) * scale;
  const double u[3][3] = {{u0.x, u1.x, e * n.x}, {u0.y, u1.y, e * n.y}, {u0.z, u1.z, e * n.z}};
  const double v[3][3] = {{v0.x, v1.x, v2.x}, {v0.y, v1.y, v2.y}, {v0.z, v1.z, v2.z}};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = u[i][0] * v[j][0] + u[i][1] * v[j][1] + u[i][2] * v[j][2];
}

// The fixed-order sum of one value per chunk: eight interleaved groups of chunks, then the groups in ascending order.
// Lane m < count of every group calls term(k, m) for its chunks; out[m] is valid after the call, for every thread.
template <typename Term>
__device__ __forceinline__ void sum_over_chunks(int chunks, int count, double (*groups)[kMoments], double *out,
                                                Term term) {
  const int tid = (int)threadIdx.x, group = tid >> 5, m = tid & 31;
  if (m < count) {
    double v = 0.0;
    for (int k = group; k < chunks; k += kSolveGroups) v += term(k, m);
    groups[group][m] = v;
  }
  __syncthreads();
  if (tid < count) {
    double v = groups[0][tid];
#pragma unroll
    for (int g = 1; g < kSolveGroups; ++g) v += groups[g][tid];
    out[tid] = v;
  }
  __syncthreads();
}

// grid (B).  The ICP bookkeeping (converged, iterations, prev_rmse) is all given or all NULL.
// The chunks' (W, means, centred moments) meet in two passes, both in the fixed order: the image's means as offsets
// from the means of its first chunk that counts anything, then every chunk's centred moments moved onto those means,
// C_k + W_k (mx_k - xm)(my_k - ym)^T.  No row that is not counted enters anywhere, and coincident points give offsets
// and moments of exactly 0.
__global__ __launch_bounds__(kSolveThreads) void k_align_solve(
    int chunks, const double *__restrict__ partials, int estimate_scale, int allow_reflection,
    double relative_rmse_thr, float *__restrict__ R, float *__restrict__ T, float *__restrict__ s,
    float *__restrict__ rmse, int32_t *__restrict__ converged, int32_t *__restrict__ iterations,
    double *__restrict__ prev_rmse) {
  __shared__ double groups[kSolveGroups][kMoments];
  __shared__ double means[kMeanSums], centred[kCentredSums];
  __shared__ int first_of_wave[kSolveWaves];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (converged && converged[b]) return;   // (the whole workgroup) frozen
  const double *pb = partials + (size_t)b * chunks * kMoments;

  int lowest = kNoRow;   // the first chunk with W > 0
  for (int k = tid; k < chunks; k += kSolveThreads)
    if (pb[(size_t)k * kMoments] > 0.0) {
      lowest = k;
      break;
    }
#pragma unroll
  for (int step = kWave / 2; step > 0; step >>= 1) lowest = min(lowest, __shfl_xor(lowest, step, kWave));
  if ((tid & (kWave - 1)) == 0) first_of_wave[tid >> 6] = lowest;
  __syncthreads();
  lowest = first_of_wave[0];
#pragma unroll
  for (int wv = 1; wv < kSolveWaves; ++wv) lowest = min(lowest, first_of_wave[wv]);
  double origin[6];   // of x and of y
#pragma unroll
  for (int k = 0; k < 6; ++k) origin[k] = lowest != kNoRow ? pb[(size_t)lowest * kMoments + 1 + k] : 0.0;

  sum_over_chunks(chunks, kMeanSums, groups, means, [&](int k, int m) {
    const double *p = pb + (size_t)k * kMoments;
    return m == 0 ? p[0] : p[0] * (p[m] - origin[m - 1]);
  });
  const double W = means[0];
  const double iw = W != 0.0 ? 1.0 / W : 0.0;
  double offset[6];   // the image's means from the origin
#pragma unroll
  for (int k = 0; k < 6; ++k) offset[k] = means[1 + k] * iw;
  sum_over_chunks(chunks, kCentredSums, groups, centred, [&](int k, int m) {
    const double *p = pb + (size_t)k * kMoments;
    double d[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) d[c] = (p[1 + c] - origin[c]) - offset[c];
    double moved;
    if (m < 9) moved = d[m / 3] * d[3 + m % 3];
    else if (m == 9) moved = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    else moved = d[3] * d[3] + d[4] * d[4] + d[5] * d[5];
    return p[7 + m] + p[0] * moved;
  });
  if (tid != 0) return;

  float *Rb = R + (size_t)b * 9, *Tb = T + (size_t)b * 3;
  double total = 0.0;
  for (int k = 0; k < kMeanSums; ++k) total += means[k];
  for (int k = 0; k < kCentredSums; ++k) total += centred[k];
  if (!(fabs(total) < (double)INFINITY)) {   // a non-finite coordinate or weight in a kept row
    for (int k = 0; k < 9; ++k) Rb[k] = NAN;
    for (int k = 0; k < 3; ++k) Tb[k] = NAN;
    s[b] = NAN;
    if (rmse) rmse[b] = NAN;
    if (converged) {
      iterations[b] += 1;
      prev_rmse[b] = NAN;
    }
    return;
  }
  if (!(W > 0.0)) {   // nothing to align
    if (converged) {   // ICP: the transform stays, the image is done
      converged[b] = 1;
      iterations[b] += 1;
      rmse[b] = 0.0f;
      prev_rmse[b] = 0.0;
      return;
    }
    for (int k = 0; k < 9; ++k) Rb[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    for (int k = 0; k < 3; ++k) Tb[k] = 0.0f;
    s[b] = 1.0f;
    if (rmse) rmse[b] = 0.0f;
    return;
  }
  double xm[3], ym[3], c[9];
  for (int k = 0; k < 3; ++k) xm[k] = origin[k] + offset[k], ym[k] = origin[3 + k] + offset[3 + k];
  for (int k = 0; k < 9; ++k) c[k] = centred[k] * iw;
  const double var_x = fmax(centred[9] * iw, 0.0);
  const double var_y = fmax(centred[10] * iw, 0.0);
  double rot[9], trace;
  rotation_of(c, allow_reflection != 0, rot, &trace);
  const double scale = (estimate_scale && var_x > 0.0) ? trace / var_x : 1.0;
  double t[3];
  for (int j = 0; j < 3; ++j) {
    double moved = 0.0;
    for (int i = 0; i < 3; ++i) moved += xm[i] * rot[3 * i + j];
    t[j] = ym[j] - scale * moved;
  }
  const double mse = fmax(scale * scale * var_x - 2.0 * scale * trace + var_y, 0.0);
  const double root = sqrt(mse);
  for (int k = 0; k < 9; ++k) Rb[k] = (float)rot[k];
  for (int k = 0; k < 3; ++k) Tb[k] = (float)t[k];
  s[b] = (float)scale;
  if (rmse) rmse[b] = (float)root;
  if (converged) {
    const int round = iterations[b] + 1;
    iterations[b] = round;
    const double before = prev_rmse[b];
    if (root == 0.0 || (round >= 2 && (before - root) / before <= relative_rmse_thr)) converged[b] = 1;
    prev_rmse[b] = root;
  }
}

// grid (blocks, B)
__global__ __launch_bounds__(256) void k_align_apply(const float *__restrict__ x, const int32_t *__restrict__ lengths,
                                                     const float *__restrict__ R, const float *__restrict__ T,
                                                     const float *__restrict__ s, int N, float *__restrict__ xt) {
  const int b = (int)blockIdx.y;
  const int nv = valid_rows(lengths, b, N);
  const float *Rb = R + (size_t)b * 9, *Tb = T + (size_t)b * 3;
  const float k = s[b];
  const float r00 = Rb[0], r01 = Rb[1], r02 = Rb[2], r10 = Rb[3], r11 = Rb[4], r12 = Rb[5], r20 = Rb[6], r21 = Rb[7],
              r22 = Rb[8];
  const float t0 = Tb[0], t1 = Tb[1], t2 = Tb[2];
  const int stride = (int)gridDim.x * 256;
  for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < N; i += stride) {
    const size_t at = ((size_t)b * N + i) * 3;
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
    if (i < nv) {
      const float a = x[at], c = x[at + 1], d = x[at + 2];
      o0 = k * (a * r00 + c * r10 + d * r20) + t0;
      o1 = k * (a * r01 + c * r11 + d * r21) + t1;
      o2 = k * (a * r02 + c * r12 + d * r22) + t2;
    }
    xt[at] = o0, xt[at + 1] = o1, xt[at + 2] = o2;
  }
}

// grid (blocks, B).  out [B,N,3]: sum bary corner of the face, 0 for a row without one.
__global__ __launch_bounds__(256) void k_align_closest(const float *__restrict__ vertices,
                                                       const int32_t *__restrict__ triangles,
                                                       const int32_t *__restrict__ face, const float *__restrict__ bary,
                                                       int N, int V, int Tn, float *__restrict__ out) {
  const int b = (int)blockIdx.y;
  const float *vb = vertices + (size_t)b * V * 3;
  const int stride = (int)gridDim.x * 256;
  for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < N; i += stride) {
    const size_t at = (size_t)b * N + i;
    const int f = face[at];
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
    if (f >= 0 && f < Tn) {
      const int v0 = triangles[3 * (size_t)f], v1 = triangles[3 * (size_t)f + 1], v2 = triangles[3 * (size_t)f + 2];
      if (v0 >= 0 && v0 < V && v1 >= 0 && v1 < V && v2 >= 0 && v2 < V) {
        const float w0 = bary[3 * at], w1 = bary[3 * at + 1], w2 = bary[3 * at + 2];
        const float *a = vb + 3 * (size_t)v0, *c = vb + 3 * (size_t)v1, *d = vb + 3 * (size_t)v2;
        o0 = w0 * a[0] + w1 * c[0] + w2 * d[0];
        o1 = w0 * a[1] + w1 * c[1] + w2 * d[1];
        o2 = w0 * a[2] + w1 * c[2] + w2 * d[2];
      }
    }
    out[3 * at] = o0, out[3 * at + 1] = o1, out[3 * at + 2] = o2;
  }
}

// grid (ceil(B / 256)).  R0 / T0 / s0: the start, or NULL for the identity.
__global__ __launch_bounds__(256) void k_align_init(const float *__restrict__ R0, const float *__restrict__ T0,
                                                    const float *__restrict__ s0, int B, float *__restrict__ R,
                                                    float *__restrict__ T, float *__restrict__ s,
                                                    float *__restrict__ rmse, int32_t *__restrict__ converged,
                                                    int32_t *__restrict__ iterations, double *__restrict__ prev_rmse) {
  const int b = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (b >= B) return;
  for (int k = 0; k < 9; ++k) R[(size_t)b * 9 + k] = R0 ? R0[(size_t)b * 9 + k] : ((k % 4 == 0) ? 1.0f : 0.0f);
  for (int k = 0; k < 3; ++k) T[(size_t)b * 3 + k] = T0 ? T0[(size_t)b * 3 + k] : 0.0f;
  s[b] = s0 ? s0[b] : 1.0f;
  rmse[b] = 0.0f;
  converged[b] = 0;
  iterations[b] = 0;
  prev_rmse[b] = 0.0;
}

inline unsigned row_blocks(int N) {
  int blocks = (N + 255) / 256;
  return (unsigned)(blocks > 4096 ? 4096 : blocks);
}

}  // namespace

// the chunks' partials [B][chunks][18] float64
size_t align_ws(int B, int N) { return align_up((size_t)B * chunks_of(N) * kMoments * sizeof(double), 256); }

int launch_align_solve(const float *x, const float *y, const int32_t *idx, int gather, const float *weights,
                       const float *sqdist, float max_sqdist, const int32_t *lengths, int B, int N, int M,
                       int estimate_scale, int allow_reflection, double relative_rmse_thr, float *R, float *T, float *s,
                       float *rmse, int32_t *converged, int32_t *iterations, double *prev_rmse, void *ws,
                       hipStream_t stream) {
  const int chunks = chunks_of(N);
  double *partials = (double *)ws;
  hipLaunchKernelGGL(k_align_moments, dim3((unsigned)chunks, (unsigned)B), dim3(kMomentThreads), 0, stream, x, y, idx,
                     gather, weights, sqdist, max_sqdist, lengths, converged, N, M, partials);
  int rc = check_launch();
  if (rc != MR_OK) return rc;
  hipLaunchKernelGGL(k_align_solve, dim3((unsigned)B), dim3(kSolveThreads), 0, stream, chunks, partials,
                     estimate_scale, allow_reflection, relative_rmse_thr, R, T, s, rmse, converged, iterations,
                     prev_rmse);
  return check_launch();
}

int launch_align_apply(const float *x, const int32_t *lengths, const float *R, const float *T, const float *s, int B,
                       int N, float *xt, hipStream_t stream) {
  hipLaunchKernelGGL(k_align_apply, dim3(row_blocks(N), (unsigned)B), dim3(256), 0, stream, x, lengths, R, T, s, N, xt);
  return check_launch();
}

int launch_align_closest_points(const float *vertices, const int32_t *triangles, const int32_t *face, const float *bary,
                                int B, int N, int V, int T, float *out, hipStream_t stream) {
  hipLaunchKernelGGL(k_align_closest, dim3(row_blocks(N), (unsigned)B), dim3(256), 0, stream, vertices, triangles, face,
                     bary, N, V, T, out);
  return check_launch();
}

int launch_align_icp_init(const float *R0, const float *T0, const float *s0, int B, float *R, float *T, float *s,
                          float *rmse, int32_t *converged, int32_t *iterations, double *prev_rmse, hipStream_t stream) {
  hipLaunchKernelGGL(k_align_init, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, R0, T0, s0, B, R, T, s, rmse,
                     converged, iterations, prev_rmse);
  return check_launch();
}

}  // namespace mr
