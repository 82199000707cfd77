// Brute-force nearest neighbour between two point clouds on gfx950, the hot path of the Chamfer distance
// (mr_nearest_forward / _backward; semantics: INTEGRATION.md, "Point-cloud losses").
//
// Per image b, for every query x_i (i < x_lengths[b]) over the targets y_j (j < y_lengths[b]):
//   sqdist_i = min_j (x_i - y_j).(x_i - y_j),   idx_i = the lowest j that attains it
// in the DIFFERENCE form only: |x|^2 + |y|^2 - 2 x.y loses every digit of a nearest distance once the clouds sit
// away from the origin (and with it MFMA is no option).  The work is VALU-bound: 3 subtractions, a product, two
// fused multiply-adds, a compare and two selects per (query, target) pair -- the first six in packed fp32, two
// queries an instruction, where a lane holds four queries -- and no memory traffic to speak of.
//
// Forward: a lane keeps `queries_per_lane` queries and their running (best distance, best index) in registers; a
// workgroup stages 256 targets at a time in LDS as three planes and every lane reads the same four targets per
// ds_read_b128 (one address for the wavefront: a broadcast).  The grid is (query blocks, target splits, B): with few
// queries and many targets -- a mesh's vertices against a scan -- the target range is cut into `splits` runs of whole
// tiles so that the chip is filled (nearest_plan, a pure host function).  A split writes one 64-bit key per query,
// (distance bits << 32) | index, to a slot of its own with a plain store; k_nearest_merge takes the unsigned minimum
// over a query's slots.  Distances are >= 0, so their bit patterns order like the values, and the index in the low
// word sends equal distances to the lowest index whatever the launch shape: no atomics, no dependence on the order
// in which workgroups finish.  Inside a split the targets are visited in ascending order with a strict '<'.
// Chamfer's per-image mean is a fixed-order sum: the pass that writes the final distances also sums its workgroup's
// into one workspace float, and k_nearest_mean adds an image's floats in a fixed order (as k_mesh_reg_sum_rows).
//
// Backward of sum_i g_i |x_i - y_idx_i|^2: a gather half, dx_i = 2 g_i (x_i - y_idx_i), and a scatter half,
// dy_j = -sum_{i: idx_i = j} 2 g_i (x_i - y_j).  The scatter runs as a gather over an inverted index built from the
// saved idx (the caller's stable sort: per destination, its queries in ascending order): eight lanes own one
// destination point, walk its list eight entries a trip and meet in a fixed butterfly.  One launch per cloud writes
// every gradient row exactly once -- both halves that land on it, when Chamfer runs both directions -- so nothing is
// zero-filled and the result is bitwise reproducible in either deterministic mode.
#include <math.h>

#include "mr_internal.h"

namespace mr {
namespace {

constexpr int kThreads = 256;          // 4 wavefronts
constexpr int kTile = 256;             // targets staged in LDS at a time, and the granularity of a split
constexpr int kWideQueries = 4;        // queries per lane once a cloud fills a workgroup of them
constexpr int kFillBlocks = 1024;      // workgroups wanted in flight: 4 per CU of the MI355X
constexpr int kLanesPerPoint = 8;      // backward: lanes per destination point
constexpr int kPointsPerBlock = kThreads / kLanesPerPoint;
static_assert(kThreads == 4 * kWave, "block_sum sums four wavefronts");
static_assert(kTile % 4 == 0, "the tile is read four targets at a time");

struct Plan {
  int splits, queries_per_lane, query_blocks, chunk;   // chunk: targets per split, whole tiles
};

inline Plan plan_of(int B, int N, int M) {
  Plan p;
  p.queries_per_lane = N >= kThreads * kWideQueries ? kWideQueries : 1;
  const int per_block = kThreads * p.queries_per_lane;
  p.query_blocks = (N + per_block - 1) / per_block;
  const int tiles = (M + kTile - 1) / kTile;
  const long long blocks = (long long)B * p.query_blocks;
  long long want = (kFillBlocks + blocks - 1) / blocks;
  if (want < 1) want = 1;
  int splits = (int)(want < tiles ? want : tiles);
  const int chunk_tiles = (tiles + splits - 1) / splits;
  p.splits = (tiles + chunk_tiles - 1) / chunk_tiles;   // no split without a tile
  p.chunk = chunk_tiles * kTile;
  return p;
}

inline unsigned merge_blocks_of(int N) { return (unsigned)((N + kThreads - 1) / kThreads); }

// rows of the last pass over the queries (the one that writes the distances): what k_nearest_mean adds per image
inline unsigned partial_rows_of(const Plan &p, int N) {
  return p.splits > 1 ? merge_blocks_of(N) : (unsigned)p.query_blocks;
}

inline size_t keys_bytes(const Plan &p, int B, int N) {
  return p.splits > 1 ? align_up((size_t)B * p.splits * N * sizeof(unsigned long long), 256) : 0;
}

__device__ __forceinline__ int valid_count(const int32_t *__restrict__ lengths, int b, int n) {
  return lengths ? min(max(lengths[b], 0), n) : n;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// The workgroup's sum of v in a fixed order, returned on every thread.  Every thread of the workgroup calls it.
__device__ __forceinline__ float block_sum(float v) {
  __shared__ float part[kThreads / kWave];
  v = wave_sum(v);
  if (lane_id() == 0) part[(int)threadIdx.x / kWave] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

constexpr unsigned long long kNoKey = ~0ull;
typedef float F2 __attribute__((ext_vector_type(2)));

// ---- forward ----------------------------------------------------------------------------------------------------
// grid (query blocks, splits, B).  keys != null (splits > 1): one key per (image, split, query) and nothing else;
// keys == null: the final sqdist / idx and, with partials, the workgroup's sum of its valid distances.
template <int Q>
__global__ __launch_bounds__(kThreads) void k_nearest(const float *__restrict__ x, const float *__restrict__ y,
                                                      const int32_t *__restrict__ x_lengths,
                                                      const int32_t *__restrict__ y_lengths, int N, int M, int chunk,
                                                      float *__restrict__ sqdist, int32_t *__restrict__ idx,
                                                      unsigned long long *__restrict__ keys,
                                                      float *__restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float sx[kTile];
  __shared__ __attribute__((aligned(16))) float sy[kTile];
  __shared__ __attribute__((aligned(16))) float sz[kTile];
  const int b = (int)blockIdx.z, split = (int)blockIdx.y;
  const int nv = valid_count(x_lengths, b, N), mv = valid_count(y_lengths, b, M);
  const float *xb = x + (size_t)b * N * 3;
  const float *yb = y + (size_t)b * M * 3;
  const int j0 = min(split * chunk, mv), j1 = min(j0 + chunk, mv);   // this split's targets, maybe none
  const int i0 = (int)blockIdx.x * (kThreads * Q) + (int)threadIdx.x;

  float px[Q], py[Q], pz[Q], best[Q];
  int bi[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = i0 + q * kThreads;
    const bool have = i < nv;
    px[q] = have ? xb[3 * (size_t)i] : 0.0f;
    py[q] = have ? xb[3 * (size_t)i + 1] : 0.0f;
    pz[q] = have ? xb[3 * (size_t)i + 2] : 0.0f;
    best[q] = INFINITY;
    bi[q] = j0;   // what a query whose every distance is NaN keeps: in range wherever the split has a target
  }

  for (int t0 = j0; t0 < j1; t0 += kTile) {   // j0, j1: the same on every thread
    const int count = min(kTile, j1 - t0);
    const int padded = (count + 3) & ~3;   // +inf beyond count: never nearer than anything
    __syncthreads();
    for (int f = (int)threadIdx.x; f < 3 * padded; f += kThreads) {
      const int j = f / 3, c = f - 3 * j;
      const float v = j < count ? yb[3 * (size_t)t0 + f] : INFINITY;
      float *plane = c == 0 ? sx : (c == 1 ? sy : sz);
      plane[j] = v;
    }
    __syncthreads();
    for (int j = 0; j < padded; j += 4) {
      const float4 tx = *reinterpret_cast<const float4 *>(&sx[j]);
      const float4 ty = *reinterpret_cast<const float4 *>(&sy[j]);
      const float4 tz = *reinterpret_cast<const float4 *>(&sz[j]);
      const float ax[4] = {tx.x, tx.y, tx.z, tx.w};
      const float ay[4] = {ty.x, ty.y, ty.z, ty.w};
      const float az[4] = {tz.x, tz.y, tz.z, tz.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if constexpr (Q % 2 == 0) {
          // two queries a step in packed fp32 (v_pk_add / v_pk_mul / v_pk_fma: both halves at the rate of one)
#pragma unroll
          for (int q = 0; q < Q; q += 2) {
            const F2 dx = F2{px[q], px[q + 1]} - ax[k], dy = F2{py[q], py[q + 1]} - ay[k];
            const F2 dz = F2{pz[q], pz[q + 1]} - az[k];
            const F2 d = dx * dx + dy * dy + dz * dz;
            if (d.x < best[q]) {   // strict, targets ascending: the lowest index of equal distances; NaN never wins
              best[q] = d.x;
              bi[q] = t0 + j + k;
            }
            if (d.y < best[q + 1]) {
              best[q + 1] = d.y;
              bi[q + 1] = t0 + j + k;
            }
          }
        } else {
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            const float dx = px[q] - ax[k], dy = py[q] - ay[k], dz = pz[q] - az[k];
            const float d = dx * dx + dy * dy + dz * dz;
            if (d < best[q]) {
              best[q] = d;
              bi[q] = t0 + j + k;
            }
          }
        }
      }
    }
  }

  float sum = 0.0f;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = i0 + q * kThreads;
    if (i >= N) continue;
    if (keys) {
      const unsigned long long key =
          (i < nv && j0 < j1) ? ((unsigned long long)__float_as_uint(best[q]) << 32) | (unsigned)bi[q] : kNoKey;
      keys[((size_t)b * gridDim.y + split) * N + i] = key;
    } else {
      const bool valid = i < nv && mv > 0;
      const float d = valid ? best[q] : 0.0f;
      if (sqdist) sqdist[(size_t)b * N + i] = d;
      idx[(size_t)b * N + i] = valid ? min(max(bi[q], 0), mv - 1) : -1;
      sum += d;
    }
  }
  if (partials) {   // (a kernel argument: the same on every thread)
    sum = block_sum(sum);
    if (threadIdx.x == 0) partials[(size_t)b * gridDim.x + blockIdx.x] = sum;
  }
}

// The unsigned minimum of a query's keys over the splits -> sqdist, idx and the workgroup's partial sum.
// grid (ceil(N / kThreads), B)
__global__ __launch_bounds__(kThreads) void k_nearest_merge(const unsigned long long *__restrict__ keys, int splits,
                                                            const int32_t *__restrict__ x_lengths,
                                                            const int32_t *__restrict__ y_lengths, int N, int M,
                                                            float *__restrict__ sqdist, int32_t *__restrict__ idx,
                                                            float *__restrict__ partials) {
  const int b = (int)blockIdx.y;
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  const int nv = valid_count(x_lengths, b, N), mv = valid_count(y_lengths, b, M);
  float d = 0.0f;
  if (i < N) {
    unsigned long long key = kNoKey;
    for (int s = 0; s < splits; ++s) {
      const unsigned long long k = keys[((size_t)b * splits + s) * N + i];
      key = k < key ? k : key;
    }
    const bool valid = i < nv && mv > 0 && key != kNoKey;
    d = valid ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
    if (sqdist) sqdist[(size_t)b * N + i] = d;
    idx[(size_t)b * N + i] = valid ? min(max((int)(unsigned)(key & 0xffffffffull), 0), mv - 1) : -1;
  }
  if (partials) {
    d = block_sum(d);
    if (threadIdx.x == 0) partials[(size_t)b * gridDim.x + blockIdx.x] = d;
  }
}

// total[b] (+)= weight * (the sum of image b's `count` partials in a fixed order) / its valid queries; a direction
// with an empty side contributes 0.  One workgroup per image.
__global__ __launch_bounds__(kThreads) void k_nearest_mean(const float *__restrict__ partials, int count,
                                                           const int32_t *__restrict__ x_lengths,
                                                           const int32_t *__restrict__ y_lengths, int N, int M,
                                                           float weight, int accumulate, float *__restrict__ total) {
  const int b = (int)blockIdx.x;
  const float *rows = partials + (size_t)b * count;
  float s = 0.0f;
  for (int r = (int)threadIdx.x; r < count; r += kThreads) s += rows[r];
  s = block_sum(s);
  if (threadIdx.x == 0) {
    const int nv = valid_count(x_lengths, b, N), mv = valid_count(y_lengths, b, M);
    const float mean = (nv > 0 && mv > 0) ? s / (float)nv : 0.0f;
    total[b] = (accumulate ? total[b] : 0.0f) + weight * mean;
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------
struct V3 {
  float x, y, z;
};

// The upstream gradient of one direction's query i: per point, or the image's (Chamfer) times weight / valid queries
struct Upstream {
  const float *__restrict__ points;   // [B, queries] or null
  float per_image;                    // used when points is null
  __device__ __forceinline__ float at(size_t i) const { return points ? points[i] : per_image; }
};

// dp[b, p] for one cloud p (Np points) against the other cloud o (No points): the gather half of the direction
// p -> o (idx_po, null when that direction did not run) plus the scatter half of the direction o -> p through its
// inverted index (order_op [B,No]: o's queries grouped by the p they chose, offsets_op [B,Np+1]; null likewise).
// Both halves add 2 g (p - o_k).  grid (ceil(Np / kPointsPerBlock), B)
__global__ __launch_bounds__(kThreads) void k_nearest_backward(
    const V3 *__restrict__ p_points, const V3 *__restrict__ o_points, const int32_t *__restrict__ p_lengths,
    const int32_t *__restrict__ o_lengths, int Np, int No, const int32_t *__restrict__ idx_po,
    const float *__restrict__ g_points_po, float weight_po, const int32_t *__restrict__ order_op,
    const int32_t *__restrict__ offsets_op, const float *__restrict__ g_points_op, float weight_op,
    const float *__restrict__ g_images, V3 *__restrict__ dp) {
  const int b = (int)blockIdx.y;
  const int p = (int)blockIdx.x * kPointsPerBlock + (int)threadIdx.x / kLanesPerPoint;
  const int sub = (int)threadIdx.x % kLanesPerPoint;
  const bool have = p < Np;   // (whole groups of eight: the butterfly below stays inside one)
  const int pv = valid_count(p_lengths, b, Np), ov = valid_count(o_lengths, b, No);
  const float gi = g_images ? g_images[b] : 0.0f;   // b = blockIdx.y: wave-uniform
  const Upstream up_po{g_points_po, pv > 0 ? gi * weight_po / (float)pv : 0.0f};
  const Upstream up_op{g_points_op, ov > 0 ? gi * weight_op / (float)ov : 0.0f};
  const V3 *ob = o_points + (size_t)b * No;
  float dx = 0.0f, dy = 0.0f, dz = 0.0f;
  if (have && p < pv) {
    const V3 me = p_points[(size_t)b * Np + p];
    if (idx_po && sub == 0) {
      const int j = idx_po[(size_t)b * Np + p];
      if ((unsigned)j < (unsigned)No) {
        const float g2 = 2.0f * up_po.at((size_t)b * Np + p);
        const V3 o = ob[j];
        dx += g2 * (me.x - o.x);
        dy += g2 * (me.y - o.y);
        dz += g2 * (me.z - o.z);
      }
    }
    if (order_op) {
      const int32_t *off = offsets_op + (size_t)b * (Np + 1);
      const int e0 = max(off[p], 0), e1 = min(off[p + 1], No);
      for (int k = e0 + sub; k < e1; k += kLanesPerPoint) {
        const int i = order_op[(size_t)b * No + k];
        if ((unsigned)i >= (unsigned)No) continue;
        const float g2 = 2.0f * up_op.at((size_t)b * No + i);
        const V3 o = ob[i];
        dx += g2 * (me.x - o.x);
        dy += g2 * (me.y - o.y);
        dz += g2 * (me.z - o.z);
      }
    }
  }
#pragma unroll
  for (int m = 1; m < kLanesPerPoint; m <<= 1) {
    dx += __shfl_xor(dx, m, kLanesPerPoint);
    dy += __shfl_xor(dy, m, kLanesPerPoint);
    dz += __shfl_xor(dz, m, kLanesPerPoint);
  }
  if (have && sub == 0) dp[(size_t)b * Np + p] = V3{dx, dy, dz};
}

}  // namespace

void nearest_plan(int B, int N, int M, int *splits, int *queries_per_lane, int *target_tile, int *workgroup) {
  const Plan p = plan_of(B, N, M);
  *splits = p.splits;
  *queries_per_lane = p.queries_per_lane;
  *target_tile = kTile;
  *workgroup = kThreads;
}

size_t nearest_ws(int B, int N, int M) {
  const Plan p = plan_of(B, N, M);
  return keys_bytes(p, B, N) + align_up((size_t)B * partial_rows_of(p, N) * sizeof(float), 256);
}

int launch_nearest_forward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B,
                           int N, int M, float *sqdist, int32_t *idx, float *total, float weight, int accumulate,
                           void *ws, hipStream_t s) {
  const Plan p = plan_of(B, N, M);
  unsigned long long *keys = p.splits > 1 ? (unsigned long long *)ws : nullptr;
  float *partials = total ? (float *)((char *)ws + keys_bytes(p, B, N)) : nullptr;
  const dim3 grid((unsigned)p.query_blocks, (unsigned)p.splits, (unsigned)B);
  float *direct = keys ? nullptr : partials;
  if (p.queries_per_lane == kWideQueries)
    hipLaunchKernelGGL(k_nearest<kWideQueries>, grid, dim3(kThreads), 0, s, x, y, x_lengths, y_lengths, N, M, p.chunk,
                       sqdist, idx, keys, direct);
  else
    hipLaunchKernelGGL(k_nearest<1>, grid, dim3(kThreads), 0, s, x, y, x_lengths, y_lengths, N, M, p.chunk, sqdist,
                       idx, keys, direct);
  int rc = check_launch();
  if (rc != MR_OK) return rc;
  if (keys) {
    hipLaunchKernelGGL(k_nearest_merge, dim3(merge_blocks_of(N), (unsigned)B), dim3(kThreads), 0, s,
                       (const unsigned long long *)keys, p.splits, x_lengths, y_lengths, N, M, sqdist, idx, partials);
    rc = check_launch();
    if (rc != MR_OK) return rc;
  }
  if (total) {
    hipLaunchKernelGGL(k_nearest_mean, dim3((unsigned)B), dim3(kThreads), 0, s, (const float *)partials,
                       (int)partial_rows_of(p, N), x_lengths, y_lengths, N, M, weight, accumulate, total);
    rc = check_launch();
  }
  return rc;
}

int launch_nearest_backward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B,
                            int N, int M, const int32_t *idx_xy, const int32_t *order_xy, const int32_t *offsets_xy,
                            const int32_t *idx_yx, const int32_t *order_yx, const int32_t *offsets_yx,
                            const float *grad_points, const float *grad_images, float x_weight, float y_weight,
                            float *dx, float *dy, hipStream_t s) {
  if (dx) {   // the gather half of x -> y and the scatter half of y -> x
    const dim3 grid((unsigned)((N + kPointsPerBlock - 1) / kPointsPerBlock), (unsigned)B);
    hipLaunchKernelGGL(k_nearest_backward, grid, dim3(kThreads), 0, s, (const V3 *)x, (const V3 *)y, x_lengths,
                       y_lengths, N, M, idx_xy, grad_points, x_weight, order_yx, offsets_yx, (const float *)nullptr,
                       y_weight, grad_images, (V3 *)dx);
    const int rc = check_launch();
    if (rc != MR_OK) return rc;
  }
  if (dy) {   // the gather half of y -> x and the scatter half of x -> y
    const dim3 grid((unsigned)((M + kPointsPerBlock - 1) / kPointsPerBlock), (unsigned)B);
    hipLaunchKernelGGL(k_nearest_backward, grid, dim3(kThreads), 0, s, (const V3 *)y, (const V3 *)x, y_lengths,
                       x_lengths, M, N, idx_yx, (const float *)nullptr, y_weight, order_xy, offsets_xy, grad_points,
                       x_weight, grad_images, (V3 *)dy);
    return check_launch();
  }
  return MR_OK;
}

}  // namespace mr
