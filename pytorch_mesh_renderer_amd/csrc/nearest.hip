// Brute-force nearest neighbour between two point clouds on gfx950, the hot path of the Chamfer distance
// (mr_nearest_forward / _backward; semantics: INTEGRATION.md, "Point-cloud losses"), and further down the same search
// from points to the triangles of a mesh (mr_nearest_triangle_forward / _backward: "point to triangle") and, last,
// from the triangles to the points (mr_nearest_point_of_triangle_forward / _backward: "triangle to point"), and the
// K-neighbour form of the point search (mr_knn_forward / _backward: "K nearest neighbours"), and the winding number
// of the mesh around every point (mr_winding_number_forward: "winding number"): the same all-pairs loop with '+' where
// the searches have 'min', and the first triangle a ray meets (mr_cast_rays_forward / _backward: "ray casting"): the
// search once more, with the watertight ray-triangle test for the distance.
//
// Per image b, for every query x_i (i < x_lengths[b]) over the targets y_j (j < y_lengths[b]):
//   sqdist_i = min_j (x_i - y_j).(x_i - y_j),   idx_i = the lowest j that attains it
// in the DIFFERENCE form only: |x|^2 + |y|^2 - 2 x.y loses every digit of a nearest distance once the clouds sit
// away from the origin (and with it MFMA is no option).  The work is VALU-bound: 3 subtractions, a product, two
// fused multiply-adds, a compare and two selects per (query, target) pair -- the first six in packed fp32, two
// queries an instruction, where a lane holds four queries -- and no memory traffic to speak of.
//
// Every search has one frame, and each piece of it stands once, under "the searches' frame" below: a lane keeps its
// queries and their running result in registers (load_queries), a workgroup stages a tile of targets in LDS
// (stage_points) and every lane reads the same targets from it (read_targets), the target range is cut
// into splits that fill the chip (plan_of, split_range) and meet through 64-bit keys (key_of, k_nearest_merge), and
// the pass that writes the final distances sums them for the mean (store_partial, k_nearest_mean).  Every backward
// has one frame too: eight lanes per gradient row (gather_rows).  Neither uses an atomic, so every result is bitwise
// reproducible whatever the launch shape, in either deterministic mode.
#include <math.h>

#include "mr_internal.h"
#include "wn_fixed.h"

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

// ---- the searches' frame: host side -----------------------------------------------------------------------------
// The grid of a search is (query blocks, target splits, B): with few queries and many targets -- a mesh's vertices
// against a scan -- the target range is cut into `splits` runs of whole tiles so that the chip is filled (the
// *_plan functions, pure host functions).
struct Plan {
  int splits, queries_per_lane, query_blocks, chunk;   // chunk: targets per split, whole tiles
};

// M targets in tiles of `tile`, `wide` queries a lane once a cloud fills a workgroup of them: the point search's
// shape by default, the triangle search's with its own two constants
inline Plan plan_of(int B, int N, int M, int tile = kTile, int wide = kWideQueries) {
  Plan p;
  p.queries_per_lane = N >= kThreads * wide ? wide : 1;
  const int per_block = kThreads * p.queries_per_lane;
  p.query_blocks = (N + per_block - 1) / per_block;
  const int tiles = (M + tile - 1) / tile;
  const long long blocks = (long long)B * p.query_blocks;
  long long want = (kFillBlocks + blocks - 1) / blocks;
  if (want < 1) want = 1;
  int splits = (int)(want < tiles ? want : tiles);
  const int chunk_tiles = (tiles + splits - 1) / splits;
  p.splits = (tiles + chunk_tiles - 1) / chunk_tiles;   // no split without a tile
  p.chunk = chunk_tiles * tile;
  return p;
}

inline dim3 search_grid(const Plan &p, int B) {
  return dim3((unsigned)p.query_blocks, (unsigned)p.splits, (unsigned)B);
}

// one thread per row of n (the merge and finish passes), and eight lanes per row of n (gather_rows)
inline unsigned row_blocks_of(int n) { return (unsigned)((n + kThreads - 1) / kThreads); }
inline dim3 rows_grid(int n, int B) { return dim3(row_blocks_of(n), (unsigned)B); }
inline dim3 groups_grid(int n, int B) {
  return dim3((unsigned)((n + kPointsPerBlock - 1) / kPointsPerBlock), (unsigned)B);
}

// A search's workspace: the triangle records | the splits' keys (splits > 1) | the partial sums of the last pass
// over the queries.  Byte offsets and the size; *_ws() and launch_*_forward() both take them from here.
struct Layout {
  size_t records, keys, partials, bytes;
};

struct Workspace {
  float4 *records;
  unsigned long long *keys;   // null without a split
  float *partials;            // null when no total is wanted
};

inline Layout layout_of(const Plan &p, int B, size_t records_bytes, size_t keys_per_split, size_t partial_rows) {
  Layout l;
  l.records = 0;
  l.keys = l.records + records_bytes;
  l.partials =
      l.keys + (p.splits > 1 ? align_up((size_t)B * p.splits * keys_per_split * sizeof(unsigned long long), 256) : 0);
  l.bytes = l.partials + align_up((size_t)B * partial_rows * sizeof(float), 256);
  return l;
}

inline Workspace carve(void *ws, const Plan &p, const Layout &l, bool want_partials) {
  Workspace w;
  w.records = (float4 *)((char *)ws + l.records);
  w.keys = p.splits > 1 ? (unsigned long long *)((char *)ws + l.keys) : nullptr;
  w.partials = want_partials ? (float *)((char *)ws + l.partials) : nullptr;
  return w;
}

// ---- the searches' frame: device side ---------------------------------------------------------------------------
__device__ __forceinline__ int valid_count(const int32_t *__restrict__ lengths, int b, int n) {
  return lengths ? min(max(lengths[b], 0), n) : n;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// The workgroup's sum of v in a fixed order, returned on every thread.  Every thread of the workgroup calls it.
template <typename T>
__device__ __forceinline__ T block_sum(T v) {
  __shared__ T part[kThreads / kWave];
  v = wave_sum(v);
  if (lane_id() == 0) part[(int)threadIdx.x / kWave] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

// Chamfer's per-image mean is a fixed-order sum: the pass that writes the final distances also sums its workgroup's
// into partials[b, blockIdx.x], and k_nearest_mean adds an image's floats in a fixed order (as k_mesh_reg_sum_rows).
// Every thread of the workgroup calls it; nothing happens without partials (a kernel argument: the same on every
// thread).
__device__ __forceinline__ void store_partial(float *__restrict__ partials, int b, float v) {
  if (!partials) return;
  v = block_sum(v);
  if (threadIdx.x == 0) partials[(size_t)b * gridDim.x + blockIdx.x] = v;
}

// A split writes one 64-bit key per query, (distance bits << 32) | index, to a slot of its own with a plain store;
// the merge takes the unsigned minimum over a query's slots.  Distances are >= 0, so their bit patterns order like
// the values, and the index in the low word sends equal distances to the lowest index whatever the launch shape: no
// atomics, no dependence on the order in which workgroups finish.  A NaN's bit pattern is above +inf's.
constexpr unsigned long long kNoKey = ~0ull;
__device__ __forceinline__ unsigned long long key_of(float d, int j) {
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j;
}
__device__ __forceinline__ float key_distance(unsigned long long key) { return __uint_as_float((unsigned)(key >> 32)); }
__device__ __forceinline__ int key_index(unsigned long long key) { return (int)(unsigned)(key & 0xffffffffull); }

// The targets [j0, j1) of split `split` among the image's n, maybe none; the same on every thread.
struct Range {
  int j0, j1;
};
__device__ __forceinline__ Range split_range(int split, int chunk, int n) {
  const int j0 = min(split * chunk, n);
  return Range{j0, min(j0 + chunk, n)};
}

// The Q queries of a lane, i0 + q kThreads of the image's points xb; zero for a padded row.
template <int Q>
__device__ __forceinline__ void load_queries(const float *__restrict__ xb, int i0, int nv, float (&px)[Q],
                                             float (&py)[Q], float (&pz)[Q]) {
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = i0 + q * kThreads;
    const bool have = i < nv;
    px[q] = have ? xb[3 * (size_t)i] : 0.0f;
    py[q] = have ? xb[3 * (size_t)i + 1] : 0.0f;
    pz[q] = have ? xb[3 * (size_t)i + 2] : 0.0f;
  }
}

// `count` points from src into the three LDS planes, `fill` from there up to `padded`.  Every thread of the
// workgroup calls it with the same arguments; the planes are the workgroup's to read when it returns.
__device__ __forceinline__ void stage_points(const float *__restrict__ src, int count, int padded, float fill,
                                             float *sx, float *sy, float *sz) {
  __syncthreads();
  for (int f = (int)threadIdx.x; f < 3 * padded; f += kThreads) {
    const int j = f / 3, c = f - 3 * j;
    const float v = j < count ? src[f] : fill;
    float *plane = c == 0 ? sx : (c == 1 ? sy : sz);
    plane[j] = v;
  }
  __syncthreads();
}

// The staged targets j .. j + 3 (j a multiple of four): every lane reads the same four targets per ds_read_b128 (one
// address for the wavefront: a broadcast).
__device__ __forceinline__ void read_targets(const float *sx, const float *sy, const float *sz, int j, float (&ax)[4],
                                             float (&ay)[4], float (&az)[4]) {
  const float4 tx = *reinterpret_cast<const float4 *>(&sx[j]);
  const float4 ty = *reinterpret_cast<const float4 *>(&sy[j]);
  const float4 tz = *reinterpret_cast<const float4 *>(&sz[j]);
  ax[0] = tx.x, ax[1] = tx.y, ax[2] = tx.z, ax[3] = tx.w;
  ay[0] = ty.x, ay[1] = ty.y, ay[2] = ty.z, ay[3] = ty.w;
  az[0] = tz.x, az[1] = tz.y, az[2] = tz.z, az[3] = tz.w;
}

typedef float F2 __attribute__((ext_vector_type(2)));

// ---- forward ----------------------------------------------------------------------------------------------------
// A lane keeps Q queries and their running (best distance, best index) in registers; a workgroup stages 256 targets
// at a time.  Inside a split the targets are visited in ascending order with a strict '<'.
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
  const float *yb = y + (size_t)b * M * 3;
  const Range run = split_range(split, chunk, mv);
  const int i0 = (int)blockIdx.x * (kThreads * Q) + (int)threadIdx.x;

  float px[Q], py[Q], pz[Q], best[Q];
  int bi[Q];
  load_queries<Q>(x + (size_t)b * N * 3, i0, nv, px, py, pz);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    best[q] = INFINITY;
    bi[q] = run.j0;   // what a query whose every distance is NaN keeps: in range wherever the split has a target
  }

  for (int t0 = run.j0; t0 < run.j1; t0 += kTile) {
    const int count = min(kTile, run.j1 - t0);
    const int padded = (count + 3) & ~3;   // +inf beyond count: never nearer than anything
    stage_points(yb + 3 * (size_t)t0, count, padded, INFINITY, sx, sy, sz);
    for (int j = 0; j < padded; j += 4) {
      float ax[4], ay[4], az[4];
      read_targets(sx, sy, sz, j, ax, ay, az);
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
      keys[((size_t)b * gridDim.y + split) * N + i] = (i < nv && run.j0 < run.j1) ? key_of(best[q], bi[q]) : kNoKey;
    } else {
      const bool valid = i < nv && mv > 0;
      const float d = valid ? best[q] : 0.0f;
      if (sqdist) sqdist[(size_t)b * N + i] = d;
      idx[(size_t)b * N + i] = valid ? min(max(bi[q], 0), mv - 1) : -1;
      sum += d;
    }
  }
  store_partial(partials, b, sum);
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
    d = valid ? key_distance(key) : 0.0f;
    if (sqdist) sqdist[(size_t)b * N + i] = d;
    idx[(size_t)b * N + i] = valid ? min(max(key_index(key), 0), mv - 1) : -1;
  }
  store_partial(partials, b, d);
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
// Backward of sum_i g_i |x_i - y_idx_i|^2: a gather half, dx_i = 2 g_i (x_i - y_idx_i), and a scatter half,
// dy_j = -sum_{i: idx_i = j} 2 g_i (x_i - y_j).  The scatter runs as a gather over an inverted index built from the
// saved idx (the caller's stable sort: per destination, its queries in ascending order).  One launch per cloud
// writes every gradient row exactly once -- both halves that land on it, when Chamfer runs both directions -- so
// nothing is zero-filled and the result is bitwise reproducible in either deterministic mode.
struct V3 {
  float x, y, z;
};

// The upstream gradient of one direction's query i: per point, or the image's (Chamfer) times weight / valid queries
struct Upstream {
  const float *__restrict__ points;   // [B, queries] or null
  float per_image;                    // used when points is null
  __device__ __forceinline__ float at(size_t i) const { return points ? points[i] : per_image; }
};

// The sum of v over the eight lanes that own one destination row, in a fixed butterfly, on each of them.
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = 1; m < kLanesPerPoint; m <<= 1) v += __shfl_xor(v, m, kLanesPerPoint);
  return v;
}

// The frame of every gather: out[b, row] = the sum over sub of what body(row, sub, dx, dy, dz) adds to (dx, dy, dz),
// for the image's `rows` rows.  Eight lanes (sub 0 .. 7) own one row, walk its list eight entries a trip -- for
// (k = e0 + sub; k < e1; k += kLanesPerPoint) -- and meet in a fixed butterfly; whole groups of eight either have a
// row or do not, so the butterfly stays inside one.  grid (ceil(rows / kPointsPerBlock), B)
template <typename Body>
__device__ __forceinline__ void gather_rows(int b, int rows, V3 *__restrict__ out, Body body) {
  const int row = (int)blockIdx.x * kPointsPerBlock + (int)threadIdx.x / kLanesPerPoint;
  const int sub = (int)threadIdx.x % kLanesPerPoint;
  const bool have = row < rows;
  float dx = 0.0f, dy = 0.0f, dz = 0.0f;
  if (have) body(row, sub, dx, dy, dz);
  dx = group_sum(dx), dy = group_sum(dy), dz = group_sum(dz);
  if (have && sub == 0) out[(size_t)b * rows + row] = V3{dx, dy, dz};
}

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
  const int pv = valid_count(p_lengths, b, Np), ov = valid_count(o_lengths, b, No);
  const float gi = g_images ? g_images[b] : 0.0f;   // b = blockIdx.y: wave-uniform
  const Upstream up_po{g_points_po, pv > 0 ? gi * weight_po / (float)pv : 0.0f};
  const Upstream up_op{g_points_op, ov > 0 ? gi * weight_op / (float)ov : 0.0f};
  const V3 *ob = o_points + (size_t)b * No;
  gather_rows(b, Np, dp, [&](int p, int sub, float &dx, float &dy, float &dz) {
    if (p >= pv) return;
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
  });
}

// ---- point to triangle ------------------------------------------------------------------------------------------
// mr_nearest_triangle_forward / _backward: per image, for every query p_i the squared distance to the nearest CLOSED
// triangle of one shared topology, the lowest face that attains it and the barycentrics of the closest point
// ("Point-cloud losses").  dist^2(p, (a, b, c)) is the least of up to four candidates -- the plane
// projection where it falls inside (det > 0, v >= 0, w >= 0, v + w <= 1) and the closest points of the segments ab,
// bc and ca (parameter clamped to [0, 1], a zero-length segment is its end point) -- each evaluated in the
// difference form relative to the first corner, |d - (beta e0 + gamma e1)|^2 with d = p - a.  A zero-area triangle is
// therefore its edges or its point: finite, never NaN.
//
// k_nt_setup gathers every image's triangles into 80-byte records (a, e0, e1, e2 = c - b, the three dot products
// and four reciprocals, formed in float64 from the float32 edges); a triangle with an index outside [0, V) becomes
// a record with a = +inf, whose every distance is +inf or NaN and never compares below the running best.  k_nt_search
// is k_nearest over those records: 128 of them staged in LDS, every lane reading the same record as four
// ds_read_b128 and a ds_read_b96 (a broadcast), one or two queries a lane -- two in packed fp32 -- ascending faces and a strict '<',
// 64-bit keys and k_nearest_merge when the faces are split.  It keeps the distance and the face only.  k_nt_finish
// evaluates the chosen face again with the SAME device functions (tri_candidates / tri_distance, compiled without
// contraction and with explicit fused multiply-adds, so that the scalar and the packed instantiation round alike):
// the distance it writes is the one that won, bit for bit.  The mean is k_nearest_mean over its partial sums.
//
// Backward (the envelope theorem: the barycentrics are constants): dp_i = 2 g_i (p_i - c_i), one row per query, and
// dv_k = -sum 2 g_i bary_ik (p_i - c_i) as a gather over the inverted index of the 3N (query, corner) entries keyed
// by vertex (gather_rows: eight lanes per vertex); p - c is d - (beta e0 + gamma e1) again.
constexpr int kTriTile = 128;          // records staged in LDS at a time (10 KB), and the granularity of a split
constexpr int kTriWideQueries = 2;     // queries per lane once a cloud fills a workgroup of them: one packed pair
constexpr int kRecWords = 5;           // 16-byte words per record
// word 0: a.xyz, 1 / det (0 unless det > 0)      word 1: e0.xyz, 1 / |e0|^2 (0 for a zero-length edge)
// word 2: e1.xyz, 1 / |e1|^2                      word 3: e2.xyz, 1 / |e2|^2         word 4: |e0|^2, e0.e1, |e1|^2, -

__device__ __forceinline__ float fma_of(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ F2 fma_of(F2 a, F2 b, F2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float clamp01(float t) { return fmaxf(fminf(t, 1.0f), 0.0f); }
__device__ __forceinline__ F2 clamp01(F2 t) { return F2{clamp01(t.x), clamp01(t.y)}; }
__device__ __forceinline__ bool inside_of(float v, float w) { return v >= 0.0f && w >= 0.0f && v + w <= 1.0f; }
__device__ __forceinline__ float where_inside(float v, float w, float d) { return inside_of(v, w) ? d : INFINITY; }
__device__ __forceinline__ F2 where_inside(F2 v, F2 w, F2 d) {
  return F2{where_inside(v.x, w.x, d.x), where_inside(v.y, w.y, d.y)};
}
__device__ __forceinline__ float lesser(float a, float b) { return a < b ? a : b; }   // b when a is NaN
__device__ __forceinline__ F2 lesser(F2 a, F2 b) { return F2{lesser(a.x, b.x), lesser(a.y, b.y)}; }
__device__ __forceinline__ float part_of(float v, int) { return v; }
__device__ __forceinline__ float part_of(F2 v, int q) { return q == 0 ? v.x : v.y; }

// The four candidates of one triangle for one (float) or two (F2) queries: squared distances and parameters.
template <typename F>
struct Candidates {
  F inside, ab, bc, ca;   // squared distances; `inside` is +inf where the projection is no candidate
  F v, w, tab, tbc, tca;
};

template <typename F>
__device__ __forceinline__ Candidates<F> tri_candidates(F px, F py, F pz, float4 r0, float4 r1, float4 r2, float4 r3,
                                                        float4 r4) {
#pragma clang fp contract(off)   // every fused multiply-add below is spelled: both instantiations round alike
  Candidates<F> c;
  const F dx = px - (F)r0.x, dy = py - (F)r0.y, dz = pz - (F)r0.z;
  const F p0 = fma_of(dz, (F)r1.z, fma_of(dy, (F)r1.y, dx * (F)r1.x));
  const F p1 = fma_of(dz, (F)r2.z, fma_of(dy, (F)r2.y, dx * (F)r2.x));
  {   // segment ab: a + t e0
    c.tab = clamp01(p0 * (F)r1.w);
    const F x = fma_of(c.tab, (F)-r1.x, dx), y = fma_of(c.tab, (F)-r1.y, dy), z = fma_of(c.tab, (F)-r1.z, dz);
    c.ab = fma_of(z, z, fma_of(y, y, x * x));
  }
  {   // segment ca, walked from a: a + t e1
    c.tca = clamp01(p1 * (F)r2.w);
    const F x = fma_of(c.tca, (F)-r2.x, dx), y = fma_of(c.tca, (F)-r2.y, dy), z = fma_of(c.tca, (F)-r2.z, dz);
    c.ca = fma_of(z, z, fma_of(y, y, x * x));
  }
  {   // segment bc: a + e0 + t e2
    const F bx = dx - (F)r1.x, by = dy - (F)r1.y, bz = dz - (F)r1.z;
    c.tbc = clamp01(fma_of(bz, (F)r3.z, fma_of(by, (F)r3.y, bx * (F)r3.x)) * (F)r3.w);
    const F x = fma_of(c.tbc, (F)-r3.x, bx), y = fma_of(c.tbc, (F)-r3.y, by), z = fma_of(c.tbc, (F)-r3.z, bz);
    c.bc = fma_of(z, z, fma_of(y, y, x * x));
  }
  {   // the plane projection a + v e0 + w e1
    c.v = fma_of(p0, (F)r4.z, -(p1 * (F)r4.y)) * (F)r0.w;
    c.w = fma_of(p1, (F)r4.x, -(p0 * (F)r4.y)) * (F)r0.w;
    const F x = fma_of(c.w, (F)-r2.x, fma_of(c.v, (F)-r1.x, dx));
    const F y = fma_of(c.w, (F)-r2.y, fma_of(c.v, (F)-r1.y, dy));
    const F z = fma_of(c.w, (F)-r2.z, fma_of(c.v, (F)-r1.z, dz));
    const F d = fma_of(z, z, fma_of(y, y, x * x));
    c.inside = r0.w > 0.0f ? where_inside(c.v, c.w, d) : (F)INFINITY;   // (r0.w: the same on every lane)
  }
  return c;
}

// The nearest candidate: +inf when none compares below it (NaN candidates are passed over).
template <typename F>
__device__ __forceinline__ F tri_distance(const Candidates<F> &c) {
  return lesser(c.ca, lesser(c.bc, lesser(c.ab, lesser(c.inside, (F)INFINITY))));
}

// Triangle t's three indices; true when it is usable: all of them in [0, V).
__device__ __forceinline__ bool usable_triangle(const int32_t *__restrict__ triangles, int t, int V, int &ia, int &ib,
                                                int &ic) {
  ia = triangles[3 * (size_t)t], ib = triangles[3 * (size_t)t + 1], ic = triangles[3 * (size_t)t + 2];
  return (unsigned)ia < (unsigned)V && (unsigned)ib < (unsigned)V && (unsigned)ic < (unsigned)V;
}

// grid (ceil(T / kThreads), B): records [B, T, kRecWords] of 16-byte words
__global__ __launch_bounds__(kThreads) void k_nt_setup(const V3 *__restrict__ vertices,
                                                       const int32_t *__restrict__ triangles, int V, int T,
                                                       float4 *__restrict__ records) {
  const int b = (int)blockIdx.y, t = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (t >= T) return;
  float4 *out = records + ((size_t)b * T + t) * kRecWords;
  int ia, ib, ic;
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (!usable_triangle(triangles, t, V, ia, ib, ic)) {
    out[0] = make_float4(INFINITY, INFINITY, INFINITY, 0.0f);   // d = p - a is -inf or NaN: never below the best
    out[1] = out[2] = out[3] = out[4] = zero;
    return;
  }
  const V3 *vb = vertices + (size_t)b * V;
  const V3 a = vb[ia], p = vb[ib], c = vb[ic];
  const float e0x = p.x - a.x, e0y = p.y - a.y, e0z = p.z - a.z;
  const float e1x = c.x - a.x, e1y = c.y - a.y, e1z = c.z - a.z;
  const float e2x = c.x - p.x, e2y = c.y - p.y, e2z = c.z - p.z;
  const double d00 = (double)e0x * e0x + (double)e0y * e0y + (double)e0z * e0z;
  const double d01 = (double)e0x * e1x + (double)e0y * e1y + (double)e0z * e1z;
  const double d11 = (double)e1x * e1x + (double)e1y * e1y + (double)e1z * e1z;
  const double d22 = (double)e2x * e2x + (double)e2y * e2y + (double)e2z * e2z;
  const double det = d00 * d11 - d01 * d01;
  out[0] = make_float4(a.x, a.y, a.z, det > 0.0 ? (float)(1.0 / det) : 0.0f);
  out[1] = make_float4(e0x, e0y, e0z, d00 > 0.0 ? (float)(1.0 / d00) : 0.0f);
  out[2] = make_float4(e1x, e1y, e1z, d11 > 0.0 ? (float)(1.0 / d11) : 0.0f);
  out[3] = make_float4(e2x, e2y, e2z, d22 > 0.0 ? (float)(1.0 / d22) : 0.0f);
  out[4] = make_float4((float)d00, (float)d01, (float)d11, 0.0f);
}

// grid (query blocks, splits, B).  keys != null (splits > 1): one key per (image, split, query) for k_nearest_merge;
// keys == null: the face, -1 for a padded query and for one no triangle compared below +inf for.
template <typename F>
__global__ __launch_bounds__(kThreads) void k_nt_search(const float *__restrict__ points,
                                                        const float4 *__restrict__ records,
                                                        const int32_t *__restrict__ lengths, int N, int T, int chunk,
                                                        int32_t *__restrict__ face,
                                                        unsigned long long *__restrict__ keys) {
  constexpr int Q = (int)(sizeof(F) / sizeof(float));
  __shared__ float4 tile[kTriTile * kRecWords];
  const int b = (int)blockIdx.z, split = (int)blockIdx.y;
  const int nv = valid_count(lengths, b, N);
  const float4 *rb = records + (size_t)b * T * kRecWords;
  const Range run = split_range(split, chunk, T);
  const int i0 = (int)blockIdx.x * (kThreads * Q) + (int)threadIdx.x;

  float qx[Q], qy[Q], qz[Q], best[Q];
  int bi[Q];
  load_queries<Q>(points + (size_t)b * N * 3, i0, nv, qx, qy, qz);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    best[q] = INFINITY;
    bi[q] = -1;
  }
  F px, py, pz;
  if constexpr (Q == 2) {
    px = F{qx[0], qx[1]};
    py = F{qy[0], qy[1]};
    pz = F{qz[0], qz[1]};
  } else {
    px = qx[0];
    py = qy[0];
    pz = qz[0];
  }

  for (int t0 = run.j0; t0 < run.j1; t0 += kTriTile) {
    const int count = min(kTriTile, run.j1 - t0);
    __syncthreads();
    for (int f = (int)threadIdx.x; f < count * kRecWords; f += kThreads) tile[f] = rb[(size_t)t0 * kRecWords + f];
    __syncthreads();
    for (int j = 0; j < count; ++j) {
      const float4 *r = &tile[j * kRecWords];   // one address for the wavefront
      const F d = tri_distance(tri_candidates<F>(px, py, pz, r[0], r[1], r[2], r[3], r[4]));
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const float dq = part_of(d, q);
        if (dq < best[q]) {   // strict, faces ascending: the lowest face of equal distances; NaN and +inf never win
          best[q] = dq;
          bi[q] = t0 + j;
        }
      }
    }
  }

#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = i0 + q * kThreads;
    if (i >= N) continue;
    const bool found = i < nv && bi[q] >= 0;
    if (keys)
      keys[((size_t)b * gridDim.y + split) * N + i] = found ? key_of(best[q], bi[q]) : kNoKey;
    else
      face[(size_t)b * N + i] = found ? bi[q] : -1;
  }
}

// One chosen (point, record) pair once more, with the searches' own functions: its distance -- the number that won,
// bit for bit -- and the barycentrics of the candidate that gave it.  False when no candidate compares below +inf.
__device__ __forceinline__ bool nt_evaluate(V3 p, const float4 *__restrict__ r, float &d, V3 &w) {
  const Candidates<float> c = tri_candidates<float>(p.x, p.y, p.z, r[0], r[1], r[2], r[3], r[4]);
  d = tri_distance(c);
  // the same chain as tri_distance, remembering whose parameters won
  float best = INFINITY, beta = 0.0f, gamma = 0.0f;
  if (c.inside < best) best = c.inside, beta = c.v, gamma = c.w;
  if (c.ab < best) best = c.ab, beta = c.tab, gamma = 0.0f;
  if (c.bc < best) best = c.bc, beta = 1.0f - c.tbc, gamma = c.tbc;
  if (c.ca < best) best = c.ca, beta = 0.0f, gamma = c.tca;
  w = V3{fmaxf(1.0f - (beta + gamma), 0.0f), beta, gamma};
  return d < INFINITY;
}

// The chosen pair of every row once more, with the search's own functions -> sqdist, chosen (-1 for a row without a
// result), the barycentrics and the workgroup's partial sum.  Point to triangle: the rows are the N points, row i
// pairs point i with the face chosen[i].  Triangle to point (kRowsAreTriangles): the rows are the T triangles, row i
// pairs triangle i with the point chosen[i].  The search never names a face or a point outside the image's.
// grid (ceil(rows / kThreads), B)
template <bool kRowsAreTriangles>
__global__ __launch_bounds__(kThreads) void k_nt_finish(const V3 *__restrict__ points,
                                                        const float4 *__restrict__ records,
                                                        const int32_t *__restrict__ lengths, int N, int T,
                                                        float *__restrict__ sqdist, int32_t *__restrict__ chosen,
                                                        V3 *__restrict__ bary, float *__restrict__ partials) {
  const int b = (int)blockIdx.y;
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  const int nv = valid_count(lengths, b, N);
  const int R = kRowsAreTriangles ? T : N;
  float d = 0.0f;
  if (i < R) {
    const size_t row = (size_t)b * R + i;
    int c = (kRowsAreTriangles || i < nv) ? chosen[row] : -1;
    const int point = kRowsAreTriangles ? c : i, f = kRowsAreTriangles ? i : c;
    V3 w;
    if ((unsigned)c >= (unsigned)(kRowsAreTriangles ? nv : T) ||
        !nt_evaluate(points[(size_t)b * N + point], records + ((size_t)b * T + f) * kRecWords, d, w)) {
      c = -1;
      d = 0.0f;
      w = V3{0.0f, 0.0f, 0.0f};
    }
    if (sqdist) sqdist[row] = d;
    chosen[row] = c;
    bary[row] = w;
  }
  store_partial(partials, b, d);
}

// p - c = d - (beta e0 + gamma e1) of the pair that row i of a saved result names (the rows: as k_nt_finish's), and
// the row's weights.  pv: the image's valid points.  False for a row without a result.
template <bool kRowsAreTriangles>
__device__ __forceinline__ bool nt_residual(const V3 *__restrict__ pb, const V3 *__restrict__ vb,
                                            const int32_t *__restrict__ triangles, const int32_t *__restrict__ cb,
                                            const V3 *__restrict__ wb, int i, int pv, int V, int T, V3 &r, V3 &w) {
  int point = i, f = i;
  if constexpr (kRowsAreTriangles) {
    point = cb[i];
    if ((unsigned)point >= (unsigned)pv) return false;
  } else {
    if (i >= pv) return false;
    f = cb[i];
    if ((unsigned)f >= (unsigned)T) return false;
  }
  int ia, ib, ic;
  if (!usable_triangle(triangles, f, V, ia, ib, ic)) return false;
  const V3 p = pb[point], a = vb[ia], e = vb[ib], c = vb[ic];
  w = wb[i];
  r.x = (p.x - a.x) - (w.y * (e.x - a.x) + w.z * (c.x - a.x));
  r.y = (p.y - a.y) - (w.y * (e.y - a.y) + w.z * (c.y - a.y));
  r.z = (p.z - a.z) - (w.y * (e.z - a.z) + w.z * (c.z - a.z));
  return true;
}

// dpoints[b, i] = 2 g_i (p_i - c_i), 0 for a row without a face.  grid (ceil(N / kThreads), B)
__global__ __launch_bounds__(kThreads) void k_nt_backward_points(
    const V3 *__restrict__ points, const V3 *__restrict__ vertices, const int32_t *__restrict__ triangles,
    const int32_t *__restrict__ lengths, int N, int V, int T, const int32_t *__restrict__ face,
    const V3 *__restrict__ bary, const float *__restrict__ g_points, const float *__restrict__ g_images,
    V3 *__restrict__ dpoints) {
  const int b = (int)blockIdx.y;
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= N) return;
  const int nv = valid_count(lengths, b, N);
  const Upstream up{g_points, (g_images && nv > 0) ? g_images[b] / (float)nv : 0.0f};
  V3 out = {0.0f, 0.0f, 0.0f}, r, w;
  if (nt_residual<false>(points + (size_t)b * N, vertices + (size_t)b * V, triangles, face + (size_t)b * N,
                         bary + (size_t)b * N, i, nv, V, T, r, w)) {
    const float g2 = 2.0f * up.at((size_t)b * N + i);
    out = V3{g2 * r.x, g2 * r.y, g2 * r.z};
  }
  dpoints[(size_t)b * N + i] = out;
}

// dvertices[b, v] = -sum over the (row, corner) entries that name v of 2 g_i bary_ik (p - c)_i: with R rows (the N
// points, or with kRowsAreTriangles the T triangles: nt_residual) order [B, 3R] holds the entries 3 i + k grouped by
// vertex, each group ascending, offsets [B, V + 1]; chosen, bary and g_rows are [B, R, ...].  The mean's upstream is
// g_images[b] over the image's valid points, with triangle rows over divisors[b] (its usable triangles).
// grid (ceil(V / kPointsPerBlock), B)
template <bool kRowsAreTriangles>
__global__ __launch_bounds__(kThreads) void k_nt_backward_vertices(
    const V3 *__restrict__ points, const V3 *__restrict__ vertices, const int32_t *__restrict__ triangles,
    const int32_t *__restrict__ lengths, int N, int V, int T, const int32_t *__restrict__ chosen,
    const V3 *__restrict__ bary, const int32_t *__restrict__ order, const int32_t *__restrict__ offsets,
    const float *__restrict__ g_rows, const float *__restrict__ g_images, const int32_t *__restrict__ divisors,
    V3 *__restrict__ dvertices) {
  const int b = (int)blockIdx.y;
  const int R = kRowsAreTriangles ? T : N;
  const int nv = valid_count(lengths, b, N);
  const int count = kRowsAreTriangles ? (g_images ? divisors[b] : 0) : nv;
  const Upstream up{g_rows, (g_images && count > 0) ? g_images[b] / (float)count : 0.0f};
  gather_rows(b, V, dvertices, [&](int v, int sub, float &dx, float &dy, float &dz) {
    const int32_t *off = offsets + (size_t)b * (V + 1);
    const int e0 = max(off[v], 0), e1 = min(off[v + 1], 3 * R);
    for (int k = e0 + sub; k < e1; k += kLanesPerPoint) {
      const int e = order[(size_t)b * 3 * R + k];
      if ((unsigned)e >= (unsigned)(3 * R)) continue;
      const int i = e / 3, corner = e - 3 * i;
      V3 r, w;
      if (!nt_residual<kRowsAreTriangles>(points + (size_t)b * N, vertices + (size_t)b * V, triangles,
                                          chosen + (size_t)b * R, bary + (size_t)b * R, i, nv, V, T, r, w))
        continue;
      const float s = -2.0f * up.at((size_t)b * R + i) * (corner == 0 ? w.x : (corner == 1 ? w.y : w.z));
      dx += s * r.x;
      dy += s * r.y;
      dz += s * r.z;
    }
  });
}

// ---- triangle to point ------------------------------------------------------------------------------------------
// mr_nearest_point_of_triangle_forward / _backward: per image, for every triangle the squared distance from the
// CLOSED triangle to the nearest valid point of the cloud, the lowest point that attains it and the barycentrics of
// the triangle's closest point to it ("Point-cloud losses").  The pair arithmetic is the one above
// (k_nt_setup's records, tri_candidates / tri_distance), so a (point, triangle) pair has the same float32 distance in
// both directions.  The roles are exchanged: a lane keeps ONE triangle's record in registers (20 of them, loaded
// once), a workgroup stages 256 of the image's valid points at a time in LDS as three planes and every lane reads
// the same point (one address for the wavefront: a broadcast) -- or the same two, points j and j + 1 in the halves
// of a packed pair against the record broadcast into both.  Ascending points and a strict '<' (inside a pair the
// lower half first), so the lowest point of equal distances wins; NaN and +inf never do; an odd last point shares
// its pair with a +inf point written into the tile.  The grid is (triangle blocks, splits, B): plan_of with the
// triangles as the queries cuts the CLOUD into `splits` runs of whole tiles, which meet through the 64-bit keys and
// k_nearest_merge.  The finish is k_nt_finish with triangle rows, the mean is k_nearest_mean over its partial sums
// with the divisor k_tp_usable counted: the usable triangles, a property of the topology.
//
// Backward: dv_k = -sum 2 g_t bary_tk (p_j(t) - c_t) is k_nt_backward_vertices with triangle rows, a gather over
// the inverted index of the 3T (triangle, corner) entries keyed by vertex; dp_j = sum_{t: index_t = j} 2 g_t
// (p_j - c_t) is a gather over the inverted index of the triangles keyed by the point they chose.
constexpr int kPointTile = 256;        // points staged in LDS at a time (3 KB), and the granularity of a split
constexpr int kPackedFrom = kPointTile;   // clouds of at least a tile are searched two points a step
static_assert(kPointTile % 2 == 0, "an odd count is padded to a pair inside the tile");

// U, the usable triangles, into counts[0 .. B).  One workgroup.
__global__ __launch_bounds__(kThreads) void k_tp_usable(const int32_t *__restrict__ triangles, int V, int T, int B,
                                                        int32_t *__restrict__ counts) {
  int n = 0;
#pragma clang loop vectorize(disable) interleave(disable)   // one small pass: two triangles a trip buys nothing
  for (int t = (int)threadIdx.x; t < T; t += kThreads) {
    int ia, ib, ic;
    n += usable_triangle(triangles, t, V, ia, ib, ic) ? 1 : 0;
  }
  const int total = block_sum(n);
  for (int b = (int)threadIdx.x; b < B; b += kThreads) counts[b] = total;
}

// grid (triangle blocks, splits, B).  keys != null (splits > 1): one key per (image, split, triangle) for
// k_nearest_merge; keys == null: the point, -1 for a triangle no point compared below +inf for.
template <typename F>
__global__ __launch_bounds__(kThreads) void k_tp_search(const float *__restrict__ points,
                                                        const float4 *__restrict__ records,
                                                        const int32_t *__restrict__ lengths, int N, int T, int chunk,
                                                        int32_t *__restrict__ index,
                                                        unsigned long long *__restrict__ keys) {
  constexpr int Q = (int)(sizeof(F) / sizeof(float));
  __shared__ __attribute__((aligned(16))) float sx[kPointTile];
  __shared__ __attribute__((aligned(16))) float sy[kPointTile];
  __shared__ __attribute__((aligned(16))) float sz[kPointTile];
  const int b = (int)blockIdx.z, split = (int)blockIdx.y;
  const int nv = valid_count(lengths, b, N);
  const float *pb = points + (size_t)b * N * 3;
  const Range run = split_range(split, chunk, nv);
  const int t = (int)blockIdx.x * kThreads + (int)threadIdx.x;

  // a lane beyond T keeps an unusable triangle's record: nothing compares below +inf
  float4 r0 = make_float4(INFINITY, INFINITY, INFINITY, 0.0f);
  float4 r1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r2 = r1, r3 = r1, r4 = r1;
  if (t < T) {
    const float4 *r = records + ((size_t)b * T + t) * kRecWords;
    r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
  }
  float best = INFINITY;
  int bi = -1;

  for (int t0 = run.j0; t0 < run.j1; t0 += kPointTile) {
    const int count = min(kPointTile, run.j1 - t0);
    const int padded = (count + Q - 1) / Q * Q;   // <= kPointTile; +inf beyond count: never nearer than anything
    stage_points(pb + 3 * (size_t)t0, count, padded, INFINITY, sx, sy, sz);
    for (int j = 0; j < padded; j += Q) {
      F px, py, pz;   // one address for the wavefront
      if constexpr (Q == 2) {
        const float2 x = *reinterpret_cast<const float2 *>(&sx[j]);
        const float2 y = *reinterpret_cast<const float2 *>(&sy[j]);
        const float2 z = *reinterpret_cast<const float2 *>(&sz[j]);
        px = F{x.x, x.y}, py = F{y.x, y.y}, pz = F{z.x, z.y};
      } else {
        px = sx[j], py = sy[j], pz = sz[j];
      }
      const F d = tri_distance(tri_candidates<F>(px, py, pz, r0, r1, r2, r3, r4));
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const float dq = part_of(d, q);
        if (dq < best) {   // strict, points ascending: the lowest point of equal distances; NaN and +inf never win
          best = dq;
          bi = t0 + j + q;
        }
      }
    }
  }

  if (t >= T) return;
  if (keys)
    keys[((size_t)b * gridDim.y + split) * T + t] = bi >= 0 ? key_of(best, bi) : kNoKey;
  else
    index[(size_t)b * T + t] = bi;
}

// dpoints[b, j] = sum over the triangles t that chose point j of 2 g_t (p_j - c_t): order [B, T] holds the triangles
// grouped by their point, each group ascending, offsets [B, N + 1].  A point nobody chose, and a padded one, get 0.
// grid (ceil(N / kPointsPerBlock), B)
__global__ __launch_bounds__(kThreads) void k_tp_backward_points(
    const V3 *__restrict__ points, const V3 *__restrict__ vertices, const int32_t *__restrict__ triangles,
    const int32_t *__restrict__ lengths, int N, int V, int T, const int32_t *__restrict__ index,
    const V3 *__restrict__ bary, const int32_t *__restrict__ order, const int32_t *__restrict__ offsets,
    const float *__restrict__ g_triangles, const float *__restrict__ g_images, const int32_t *__restrict__ divisors,
    V3 *__restrict__ dpoints) {
  const int b = (int)blockIdx.y;
  const int nv = valid_count(lengths, b, N);
  const int count = g_images ? divisors[b] : 0;
  const Upstream up{g_triangles, (g_images && count > 0) ? g_images[b] / (float)count : 0.0f};
  gather_rows(b, N, dpoints, [&](int p, int sub, float &dx, float &dy, float &dz) {
    if (p >= nv) return;
    const int32_t *off = offsets + (size_t)b * (N + 1);
    const int e0 = max(off[p], 0), e1 = min(off[p + 1], T);
    for (int k = e0 + sub; k < e1; k += kLanesPerPoint) {
      const int t = order[(size_t)b * T + k];
      V3 r, w;
      if ((unsigned)t >= (unsigned)T || index[(size_t)b * T + t] != p ||
          !nt_residual<true>(points + (size_t)b * N, vertices + (size_t)b * V, triangles, index + (size_t)b * T,
                             bary + (size_t)b * T, t, nv, V, T, r, w))
        continue;
      const float g2 = 2.0f * up.at((size_t)b * T + t);
      dx += g2 * r.x;
      dy += g2 * r.y;
      dz += g2 * r.z;
    }
  });
}

// ---- K nearest neighbours ---------------------------------------------------------------------------------------
// mr_knn_forward / _backward: per image, for every query x_i the K targets y_j with the K smallest 64-bit keys
// (bits of (x_i - y_j).(x_i - y_j) << 32) | j, in ascending key order ("K nearest neighbours").  The
// search is k_nearest's -- targets broadcast from LDS, the difference form, splits of whole tiles (plan_of) -- with
// the running (best, index) pair replaced by a sorted LIST of C keys per query that lives in registers: C, the
// capacity, is K rounded up to 4, 8, 16 or 32 and a template parameter, every subscript of the list is a constant
// after unrolling (a runtime subscript would send it to scratch), and the list is truncated to K on output.  A new
// key is compared with the list's worst first; only a winner replaces it and walks the compare-exchange chain down
// (C - 1 steps of one 64-bit compare and four selects).  Any lane of a wavefront that inserts makes all 64 walk it.
// Equal distances order by index and a NaN's bit pattern is above +inf's, so a NaN sorts after every number and the
// result depends on neither the capacity nor the launch shape; the distance is spelled with explicit fused
// multiply-adds so that the scalar and the packed instantiations round alike (as tri_candidates).  A split writes
// its K keys per query to the workspace, k_knn_merge keeps the K smallest of splits x K with the same list.
//
// Backward of sum_ik g_ik |x_i - y_idx_ik|^2: gather_rows again; a query's row walks its own K slots, a target's
// row the inverted index of the flattened [N K] indices (entry e belongs to query e / K).  Slots with idx -1 or a
// distance that is not finite contribute nothing.
constexpr int kKnnMaxK = 32;
constexpr int knn_wide_queries(int C) { return C <= 4 ? 4 : (C <= 8 ? 2 : 1); }   // 2 C VGPRs of keys a query
inline int knn_capacity_of(int K) { return K <= 4 ? 4 : (K <= 8 ? 8 : (K <= 16 ? 16 : 32)); }
inline Plan knn_plan_of(int B, int N, int M, int K) {
  return plan_of(B, N, M, kTile, knn_wide_queries(knn_capacity_of(K)));
}

// The C smallest keys offered so far, ascending; kNoKey where fewer were offered.
template <int C>
struct KeyList {
  unsigned long long k[C];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int s = 0; s < C; ++s) k[s] = kNoKey;
  }
  __device__ __forceinline__ void offer(unsigned long long key) {
    if (key < k[C - 1]) {   // most keys stop here
      k[C - 1] = key;
#pragma unroll
      for (int s = C - 1; s > 0; --s) {
        const unsigned long long below = k[s - 1], above = k[s];
        const bool swap = above < below;
        k[s - 1] = swap ? above : below;
        k[s] = swap ? below : above;
      }
    }
  }
};

template <typename F>
__device__ __forceinline__ F knn_distance(F px, F py, F pz, float ax, float ay, float az) {
#pragma clang fp contract(off)   // the fused multiply-adds are spelled: every instantiation rounds alike
  const F dx = px - (F)ax, dy = py - (F)ay, dz = pz - (F)az;
  return fma_of(dz, dz, fma_of(dy, dy, dx * dx));
}

// Slot k of a query's final list -> sqdist, idx: (0, -1) for a padded row and beyond the image's valid targets
__device__ __forceinline__ void knn_write(unsigned long long key, bool row_valid, int k, int mv,
                                          float *__restrict__ sqdist, int32_t *__restrict__ idx, size_t at) {
  const bool valid = row_valid && k < mv && key != kNoKey;
  const float d = key_distance(key);
  sqdist[at] = valid ? (d != d ? INFINITY : d) : 0.0f;
  idx[at] = valid ? min(key_index(key), mv - 1) : -1;
}

// grid (query blocks, splits, B).  keys != null (splits > 1): K keys per (image, split, query), [B, splits, K, N];
// keys == null: the final sqdist / idx [B, N, K].
template <int C, int Q>
__global__ __launch_bounds__(kThreads) void k_knn(const float *__restrict__ x, const float *__restrict__ y,
                                                  const int32_t *__restrict__ x_lengths,
                                                  const int32_t *__restrict__ y_lengths, int N, int M, int K, int chunk,
                                                  float *__restrict__ sqdist, int32_t *__restrict__ idx,
                                                  unsigned long long *__restrict__ keys) {
  __shared__ __attribute__((aligned(16))) float sx[kTile];
  __shared__ __attribute__((aligned(16))) float sy[kTile];
  __shared__ __attribute__((aligned(16))) float sz[kTile];
  const int b = (int)blockIdx.z, split = (int)blockIdx.y;
  const int nv = valid_count(x_lengths, b, N), mv = valid_count(y_lengths, b, M);
  const float *yb = y + (size_t)b * M * 3;
  const Range run = split_range(split, chunk, mv);
  const int i0 = (int)blockIdx.x * (kThreads * Q) + (int)threadIdx.x;

  float px[Q], py[Q], pz[Q];
  KeyList<C> list[Q];
  load_queries<Q>(x + (size_t)b * N * 3, i0, nv, px, py, pz);
#pragma unroll
  for (int q = 0; q < Q; ++q) list[q].clear();

  for (int t0 = run.j0; t0 < run.j1; t0 += kTile) {
    const int count = min(kTile, run.j1 - t0);
    const int padded = (count + 3) & ~3;   // staged as zeros beyond count and never offered
    stage_points(yb + 3 * (size_t)t0, count, padded, 0.0f, sx, sy, sz);
    for (int j = 0; j < padded; j += 4) {
      float ax[4], ay[4], az[4];
      read_targets(sx, sy, sz, j, ax, ay, az);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (j + k < count) {   // (the same on every thread)
          const int t = t0 + j + k;
          if constexpr (Q % 2 == 0) {
#pragma unroll
            for (int q = 0; q < Q; q += 2) {
              const F2 d = knn_distance(F2{px[q], px[q + 1]}, F2{py[q], py[q + 1]}, F2{pz[q], pz[q + 1]}, ax[k],
                                        ay[k], az[k]);
              list[q].offer(key_of(d.x, t));
              list[q + 1].offer(key_of(d.y, t));
            }
          } else {
#pragma unroll
            for (int q = 0; q < Q; ++q)
              list[q].offer(key_of(knn_distance(px[q], py[q], pz[q], ax[k], ay[k], az[k]), t));
          }
        }
      }
    }
  }

#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = i0 + q * kThreads;
    if (i >= N) continue;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      if (k < K) {
        if (keys)
          keys[(((size_t)b * gridDim.y + split) * K + k) * N + i] = i < nv ? list[q].k[k] : kNoKey;
        else
          knn_write(list[q].k[k], i < nv, k, mv, sqdist, idx, ((size_t)b * N + i) * K + k);
      }
    }
  }
}

// The K smallest of a query's splits x K keys -> sqdist, idx.  grid (ceil(N / kThreads), B)
template <int C>
__global__ __launch_bounds__(kThreads) void k_knn_merge(const unsigned long long *__restrict__ keys, int splits,
                                                        const int32_t *__restrict__ x_lengths,
                                                        const int32_t *__restrict__ y_lengths, int N, int M, int K,
                                                        float *__restrict__ sqdist, int32_t *__restrict__ idx) {
  const int b = (int)blockIdx.y;
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= N) return;
  const int nv = valid_count(x_lengths, b, N), mv = valid_count(y_lengths, b, M);
  KeyList<C> list;
  list.clear();
  if (i < nv)
    for (int s = 0; s < splits; ++s)
      for (int k = 0; k < K; ++k) list.offer(keys[(((size_t)b * splits + s) * K + k) * N + i]);
#pragma unroll
  for (int k = 0; k < C; ++k) {
    if (k < K) knn_write(list.k[k], i < nv, k, mv, sqdist, idx, ((size_t)b * N + i) * K + k);
  }
}

// dp[b, p] for one cloud p (Np points) against the other cloud o (No points), over the saved sqdist / idx / grad
// [B, N, K] of N queries: the sum of 2 g_e (p - o_e) over the row's entries e.  kTargets false: p is the queries'
// cloud (Np == N), row p's entries are its own K slots and o_e = y[idx_e].  kTargets true: p is the targets' cloud,
// the entries are order[offsets[p] .. offsets[p + 1]) of the inverted index (order [B, N K], offsets [B, Np + 1]) and
// o_e = x[e / K].  grid (ceil(Np / kPointsPerBlock), B)
template <bool kTargets>
__global__ __launch_bounds__(kThreads) void k_knn_backward(
    const V3 *__restrict__ p_points, const V3 *__restrict__ o_points, const int32_t *__restrict__ p_lengths,
    const int32_t *__restrict__ o_lengths, int Np, int No, int N, int K, const float *__restrict__ sqdist,
    const int32_t *__restrict__ idx, const int32_t *__restrict__ order, const int32_t *__restrict__ offsets,
    const float *__restrict__ grad, V3 *__restrict__ dp) {
  const int b = (int)blockIdx.y;
  const int pv = valid_count(p_lengths, b, Np), ov = valid_count(o_lengths, b, No);
  const int entries = N * K;   // (below 2^31: mr_knn_*'s limits)
  const size_t base = (size_t)b * entries;
  const V3 *ob = o_points + (size_t)b * No;
  gather_rows(b, Np, dp, [&](int p, int sub, float &dx, float &dy, float &dz) {
    if (p >= pv) return;
    const V3 me = p_points[(size_t)b * Np + p];
    int e0 = p * K, e1 = e0 + K;
    if constexpr (kTargets) {
      const int32_t *off = offsets + (size_t)b * (Np + 1);
      e0 = max(off[p], 0), e1 = min(off[p + 1], entries);
    }
    for (int k = e0 + sub; k < e1; k += kLanesPerPoint) {
      int e = k, other;
      if constexpr (kTargets) {
        e = order[base + k];
        if ((unsigned)e >= (unsigned)entries || idx[base + e] != p) continue;
        other = e / K;
      } else {
        other = idx[base + e];
      }
      if ((unsigned)other >= (unsigned)ov) continue;
      if (!(sqdist[base + e] < INFINITY)) continue;   // a distance that is +inf or NaN has no gradient
      const float g2 = 2.0f * grad[base + e];
      const V3 o = ob[other];
      dx += g2 * (me.x - o.x);
      dy += g2 * (me.y - o.y);
      dz += g2 * (me.z - o.z);
    }
  });
}

// ---- winding number ---------------------------------------------------------------------------------------------
// mr_winding_number_forward: per image, for every query p the generalized winding number of the mesh around it
// (Jacobson et al. 2013; INTEGRATION.md, "Point-cloud losses"): the sum over the usable triangles of the signed solid
// angle seen from p over 4 pi, with a = va - p, b = vb - p, c = vc - p (Van Oosterom and Strackee)
//   num = a . (b x c),  den = |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|,  t = 2 atan2(num, den) / (4 pi),  |t| <= 0.5.
// It is the searches' all-pairs loop with '+' where they have 'min', on the searches' frame: k_wn_setup gathers every
// image's triangles into 48-byte records (the three corners; the spare lane of the first word says whether the
// triangle is usable: every index in [0, V) and no two equal), k_wn_sum stages 128 of them in LDS, every lane reads
// the same record as three 16-byte reads (a ds_read_b128 and two ds_read_b96, the spare lanes of the last two words
// being unused: one address for the wavefront, a broadcast) and keeps one query, or two in packed fp32, with their
// sums in registers.  The sum is in 64-bit fixed point (wn_fixed.h), so it is the same number whatever the order and the
// launch shape: with splits > 1 every (image, split, query) writes its integer partial with a plain store and
// k_wn_merge adds them -- no atomics, no flags, stream order alone.  A query that met a non-finite num or den (a NaN
// or infinite point, a NaN vertex of a usable triangle, an overflow) is poisoned: NaN out, kWnPoisoned between the
// splits.  wn_terms is compiled without contraction and with explicit fused multiply-adds, as tri_candidates is, and
// the square roots and the arctangent are taken half by half, so the scalar and the packed instantiation round alike.
constexpr int kWnRecWords = 3;         // 16-byte words per record: a.xyz, usable | b.xyz, - | c.xyz, -
constexpr float kInvTwoPi = 0.15915494309189535f;

__device__ __forceinline__ float root_of(float v) { return __builtin_amdgcn_sqrtf(v); }   // v_sqrt_f32: 1 ulp
__device__ __forceinline__ F2 root_of(F2 v) { return F2{root_of(v.x), root_of(v.y)}; }
// atan2(num, den) / (2 pi), kept within the +-0.5 the fixed-point format counts on (float(pi) is above pi)
__device__ __forceinline__ float turn_of(float num, float den) {
  return fminf(fmaxf(atan2f(num, den) * kInvTwoPi, -0.5f), 0.5f);
}
__device__ __forceinline__ F2 turn_of(F2 num, F2 den) { return F2{turn_of(num.x, den.x), turn_of(num.y, den.y)}; }

__device__ __forceinline__ float where(bool keep, float v) { return keep ? v : 0.0f; }
__device__ __forceinline__ F2 where(bool keep, F2 v) { return F2{where(keep, v.x), where(keep, v.y)}; }

// num and den of one triangle (its record's three words) for one (float) or two (F2) queries.
template <typename F>
__device__ __forceinline__ void wn_terms(F px, F py, F pz, float4 r0, float4 r1, float4 r2, F &num, F &den) {
#pragma clang fp contract(off)   // every fused multiply-add below is spelled: both instantiations round alike
  const F ax = (F)r0.x - px, ay = (F)r0.y - py, az = (F)r0.z - pz;
  const F bx = (F)r1.x - px, by = (F)r1.y - py, bz = (F)r1.z - pz;
  const F cx = (F)r2.x - px, cy = (F)r2.y - py, cz = (F)r2.z - pz;
  const F nx = fma_of(by, cz, -(bz * cy)), ny = fma_of(bz, cx, -(bx * cz)), nz = fma_of(bx, cy, -(by * cx));
  num = fma_of(az, nz, fma_of(ay, ny, ax * nx));
  const F la = root_of(fma_of(az, az, fma_of(ay, ay, ax * ax)));
  const F lb = root_of(fma_of(bz, bz, fma_of(by, by, bx * bx)));
  const F lc = root_of(fma_of(cz, cz, fma_of(cy, cy, cx * cx)));
  const F ab = fma_of(az, bz, fma_of(ay, by, ax * bx));
  const F bc = fma_of(bz, cz, fma_of(by, cy, bx * cx));
  const F ca = fma_of(cz, az, fma_of(cy, ay, cx * ax));
  den = fma_of(ca, lb, fma_of(bc, la, fma_of(ab, lc, la * lb * lc)));
}

// grid (ceil(T / kThreads), B): records [B, T, kWnRecWords] of 16-byte words.  kFiniteOnly (the ray caster's rule): a
// triangle with a corner that is not finite is skipped too.
template <bool kFiniteOnly>
__global__ __launch_bounds__(kThreads) void k_wn_setup(const V3 *__restrict__ vertices,
                                                       const int32_t *__restrict__ triangles, int V, int T,
                                                       float4 *__restrict__ records) {
  const int b = (int)blockIdx.y, t = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (t >= T) return;
  float4 *out = records + ((size_t)b * T + t) * kWnRecWords;
  int ia, ib, ic;
  bool usable = usable_triangle(triangles, t, V, ia, ib, ic) && ia != ib && ib != ic && ic != ia;
  V3 a = {0.0f, 0.0f, 0.0f}, p = a, c = a;
  if (usable) {
    const V3 *vb = vertices + (size_t)b * V;
    a = vb[ia], p = vb[ib], c = vb[ic];
    if constexpr (kFiniteOnly) {
      // x * 0 is NaN for an infinite or NaN x
      const float sum = ((a.x * 0.0f + a.y * 0.0f) + (a.z * 0.0f + p.x * 0.0f)) + ((p.y * 0.0f + p.z * 0.0f) +
                        (c.x * 0.0f + c.y * 0.0f)) + c.z * 0.0f;
      usable = sum == 0.0f;
    }
  }
  if (!usable) {
    out[0] = out[1] = out[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // skipped: contributes nothing
    return;
  }
  out[0] = make_float4(a.x, a.y, a.z, 1.0f);
  out[1] = make_float4(p.x, p.y, p.z, 0.0f);
  out[2] = make_float4(c.x, c.y, c.z, 0.0f);
}

// grid (query blocks, splits, B).  partials != null (splits > 1): one 64-bit partial per (image, split, query) for
// k_wn_merge, 0 for a padded query; partials == null: w itself.
template <typename F>
__global__ __launch_bounds__(kThreads) void k_wn_sum(const float *__restrict__ points,
                                                     const float4 *__restrict__ records,
                                                     const int32_t *__restrict__ lengths, int N, int T, int chunk,
                                                     float *__restrict__ w, long long *__restrict__ partials) {
  constexpr int Q = (int)(sizeof(F) / sizeof(float));
  __shared__ float4 tile[kTriTile * kWnRecWords];
  const int b = (int)blockIdx.z, split = (int)blockIdx.y;
  const int nv = valid_count(lengths, b, N);
  const float4 *rb = records + (size_t)b * T * kWnRecWords;
  const Range run = split_range(split, chunk, T);
  const int i0 = (int)blockIdx.x * (kThreads * Q) + (int)threadIdx.x;

  float qx[Q], qy[Q], qz[Q];
  load_queries<Q>(points + (size_t)b * N * 3, i0, nv, qx, qy, qz);
  F px, py, pz;
  if constexpr (Q == 2) {
    px = F{qx[0], qx[1]};
    py = F{qy[0], qy[1]};
    pz = F{qz[0], qz[1]};
  } else {
    px = qx[0];
    py = qy[0];
    pz = qz[0];
  }
  long long sum[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) sum[q] = 0;
  F bad = (F)0.0f;   // 0, or NaN once a num or a den was not finite

  for (int t0 = run.j0; t0 < run.j1; t0 += kTriTile) {
    const int count = min(kTriTile, run.j1 - t0);
    __syncthreads();
    for (int f = (int)threadIdx.x; f < count * kWnRecWords; f += kThreads)
      tile[f] = rb[(size_t)t0 * kWnRecWords + f];
    __syncthreads();
    for (int j = 0; j < count; ++j) {
      const float4 *r = &tile[j * kWnRecWords];   // one address for the wavefront
      const float4 r0 = r[0];
      F num, den;
      wn_terms<F>(px, py, pz, r0, r[1], r[2], num, den);
      // a skipped triangle (the same on every lane) is atan2(0, 0) = 0: selects, no branch between the LDS reads
      num = where(r0.w != 0.0f, num), den = where(r0.w != 0.0f, den);
      bad = fma_of(num, (F)0.0f, fma_of(den, (F)0.0f, bad));   // x * 0 is NaN for an infinite or NaN x
      const F turn = turn_of(num, den);
#pragma unroll
      for (int q = 0; q < Q; ++q) sum[q] += wn_to_fixed(part_of(turn, q));
    }
  }

#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = i0 + q * kThreads;
    if (i >= N) continue;
    const bool valid = i < nv, poisoned = part_of(bad, q) != 0.0f;
    if (partials)
      partials[((size_t)b * gridDim.y + split) * N + i] = !valid ? 0 : (poisoned ? kWnPoisoned : sum[q]);
    else
      w[(size_t)b * N + i] = !valid ? 0.0f : (poisoned ? __int_as_float(0x7fc00000) : wn_to_float(sum[q]));
  }
}

// The sum of a query's partials over the splits -> w; NaN when one of them is poisoned, 0 for a padded query.
// grid (ceil(N / kThreads), B)
__global__ __launch_bounds__(kThreads) void k_wn_merge(const long long *__restrict__ partials, int splits,
                                                       const int32_t *__restrict__ lengths, int N,
                                                       float *__restrict__ w) {
  const int b = (int)blockIdx.y;
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= N) return;
  long long sum = 0;
  bool poisoned = false;
  for (int s = 0; s < splits; ++s) {
    const long long part = partials[((size_t)b * splits + s) * N + i];
    poisoned |= part == kWnPoisoned;
    sum += poisoned ? 0 : part;
  }
  const bool valid = i < valid_count(lengths, b, N);
  w[(size_t)b * N + i] = !valid ? 0.0f : (poisoned ? __int_as_float(0x7fc00000) : wn_to_float(sum));
}

// ---- ray casting ------------------------------------------------------------------------------------------------
// mr_cast_rays_forward / _backward: per image, for every ray (o, d) the first triangle of the mesh it meets, the
// parameter t of the hit point o + t d (d is NOT normalised) and its barycentrics, by the watertight test of Woop,
// Benthin and Wald (2013); the definition stands in include/mesh_raster.h and INTEGRATION.md, "Point-cloud losses".
// It is k_nt_search's all-pairs loop over k_wn_setup's 48-byte corner records (with kFiniteOnly: a non-finite corner
// skips the triangle too): 128 records staged in LDS, every lane reads the same record (a broadcast) and keeps one
// ray, or two in packed fp32.  A ray's axis choice (kx, ky, kz) is per-lane data and reaches the corners through
// selects (pick_of): the 2 x 3 shear matrix would need its fma chain to END on the inexact product -S p[kz], and which
// column that is differs from lane to lane, so a fixed chain rounds twice where the definition rounds once.  The
// common path of a pair is nine subtractions, the selects, six fused multiply-adds, six products, three differences
// and one sign test (ray_edges, compiled without contraction: the neighbour across a shared edge computes the exact
// negative); det, T, the division, the interval and the float64 recomputation of exact zeros (ray_accept, scalar code
// per ray) sit behind a branch that a skipped record and a dead ray never take.  Faces ascending with a strict '<':
// the lowest face of equal t.  t >= t_min >= 0 and -0 is stored as +0, so the bits of t order like the values and
// the splits meet through key_of / k_nearest_merge.  k_ray_finish evaluates the chosen pair once more with the SAME
// two functions -- their arithmetic is IEEE-exact operation by operation, so the scalar and the packed instantiation
// agree bit for bit -- and writes t, face and bary: a ray's t is the same whatever the split or the batch.
//
// Backward, the face held fixed: with n = (b - a) x (c - a) and g = n / (n . d),  dt/do = -g,  dt/dd = -t g,
// dt/dv_k = bary_k g; 0 where n . d is 0 or g is not finite.  One row per ray for the first two, a gather over the
// inverted index of the 3N (ray, corner) entries keyed by vertex for the third (gather_rows), as k_nt_backward_*.
struct Ray {
  float ox, oy, oz;   // the origin
  float sx, sy, sz;   // d[kx] / d[kz], d[ky] / d[kz], 1 / d[kz]
  int kx, ky, kz;
  bool live;          // false: a padded row, a non-finite origin or direction, a zero direction -- never hits
};

__device__ __forceinline__ bool finite3(V3 v) { return (v.x * 0.0f + v.y * 0.0f) + v.z * 0.0f == 0.0f; }
__device__ __forceinline__ float pick(int k, float x, float y, float z) { return k == 0 ? x : (k == 1 ? y : z); }

__device__ __forceinline__ Ray ray_of(V3 o, V3 d, bool have) {
  Ray r;
  const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
  const float m = fmaxf(ax, fmaxf(ay, az));
  r.live = have && finite3(o) && finite3(d) && m > 0.0f;
  r.kz = ax == m ? 0 : (ay == m ? 1 : 2);   // the first axis that attains max |d_k|
  int kx = r.kz == 2 ? 0 : r.kz + 1, ky = kx == 2 ? 0 : kx + 1;
  const float dz = pick(r.kz, d.x, d.y, d.z);
  if (dz < 0.0f) {
    const int k = kx;
    kx = ky, ky = k;
  }
  r.kx = kx, r.ky = ky;
  r.sx = r.live ? pick(kx, d.x, d.y, d.z) / dz : 0.0f;
  r.sy = r.live ? pick(ky, d.x, d.y, d.z) / dz : 0.0f;
  r.sz = r.live ? 1.0f / dz : 0.0f;
  r.ox = r.live ? o.x : 0.0f, r.oy = r.live ? o.y : 0.0f, r.oz = r.live ? o.z : 0.0f;
  return r;
}

// One (float) or two (F2) rays of a lane as ray_edges takes them: -Sx, -Sy and the origin per half, the axes per ray.
template <typename F>
struct RayLanes {
  F ox, oy, oz, nsx, nsy;
  int kx[sizeof(F) / sizeof(float)], ky[sizeof(F) / sizeof(float)], kz[sizeof(F) / sizeof(float)];
};

__device__ __forceinline__ void set_part(float &v, int, float x) { v = x; }
__device__ __forceinline__ void set_part(F2 &v, int q, float x) {
  if (q == 0)
    v.x = x;
  else
    v.y = x;
}

template <typename F>
__device__ __forceinline__ void set_ray(RayLanes<F> &lanes, int q, const Ray &r) {
  set_part(lanes.ox, q, r.ox), set_part(lanes.oy, q, r.oy), set_part(lanes.oz, q, r.oz);
  set_part(lanes.nsx, q, -r.sx), set_part(lanes.nsy, q, -r.sy);
  lanes.kx[q] = r.kx, lanes.ky[q] = r.ky, lanes.kz[q] = r.kz;
}

__device__ __forceinline__ float pick_of(const int *k, float x, float y, float z) { return pick(k[0], x, y, z); }
__device__ __forceinline__ F2 pick_of(const int *k, F2 x, F2 y, F2 z) {
  return F2{pick(k[0], x.x, y.x, z.x), pick(k[1], x.y, y.y, z.y)};
}

// The sheared corners and the edge functions of one triangle (its record's three words) for one or two rays.
template <typename F>
struct RayEdges {
  F ax, ay, bx, by, cx, cy;   // Px = fma(-Sx, p[kz], p[kx]), Py = fma(-Sy, p[kz], p[ky]) with p = corner - o
  F ak, bk, ck;               // p[kz]: Pz = Sz p[kz] is formed by ray_accept
  F u, v, w;
};

template <typename F>
__device__ __forceinline__ RayEdges<F> ray_edges(const RayLanes<F> &ray, float4 r0, float4 r1, float4 r2) {
#pragma clang fp contract(off)   // U, V, W: two rounded products and one rounded difference each, never fused
  RayEdges<F> e;
  const F pax = (F)r0.x - ray.ox, pay = (F)r0.y - ray.oy, paz = (F)r0.z - ray.oz;
  const F pbx = (F)r1.x - ray.ox, pby = (F)r1.y - ray.oy, pbz = (F)r1.z - ray.oz;
  const F pcx = (F)r2.x - ray.ox, pcy = (F)r2.y - ray.oy, pcz = (F)r2.z - ray.oz;
  e.ak = pick_of(ray.kz, pax, pay, paz);
  e.bk = pick_of(ray.kz, pbx, pby, pbz);
  e.ck = pick_of(ray.kz, pcx, pcy, pcz);
  e.ax = fma_of(ray.nsx, e.ak, pick_of(ray.kx, pax, pay, paz));
  e.ay = fma_of(ray.nsy, e.ak, pick_of(ray.ky, pax, pay, paz));
  e.bx = fma_of(ray.nsx, e.bk, pick_of(ray.kx, pbx, pby, pbz));
  e.by = fma_of(ray.nsy, e.bk, pick_of(ray.ky, pbx, pby, pbz));
  e.cx = fma_of(ray.nsx, e.ck, pick_of(ray.kx, pcx, pcy, pcz));
  e.cy = fma_of(ray.nsy, e.ck, pick_of(ray.ky, pcx, pcy, pcz));
  e.u = e.cx * e.by - e.cy * e.bx;
  e.v = e.ax * e.cy - e.ay * e.cx;
  e.w = e.bx * e.ay - e.by * e.ax;
  return e;
}

// True when some edge function is below 0 and some above: the pair is rejected.  A NaN is neither.
template <typename T>
__device__ __forceinline__ bool mixed_signs(T u, T v, T w) {
  return (u < 0 || v < 0 || w < 0) && (u > 0 || v > 0 || w > 0);
}

struct RayHit {
  float t, u, v, w;   // u, v, w: the barycentrics
};

// Everything after the edge functions for part q of e, in scalar code: the float64 recomputation when an edge function
// is exactly 0, the sign test, det, T, the division and the interval.  True: the pair is accepted.
template <typename F>
__device__ __forceinline__ bool ray_accept(const RayEdges<F> &e, int q, float sz, float tmin, float tmax, RayHit &h) {
#pragma clang fp contract(off)
  float U = part_of(e.u, q), V = part_of(e.v, q), W = part_of(e.w, q);
  if (U == 0.0f || V == 0.0f || W == 0.0f) {
    // the products of two floats are exact in float64, so the signs of the differences are
    const double ax = part_of(e.ax, q), ay = part_of(e.ay, q), bx = part_of(e.bx, q), by = part_of(e.by, q);
    const double cx = part_of(e.cx, q), cy = part_of(e.cy, q);
    const double u = cx * by - cy * bx, v = ax * cy - ay * cx, w = bx * ay - by * ax;
    if (mixed_signs(u, v, w)) return false;
    U = (float)u, V = (float)v, W = (float)w;
  } else if (mixed_signs(U, V, W)) {
    return false;
  }
  const float det = (U + V) + W;
  if (det == 0.0f) return false;
  const float az = sz * part_of(e.ak, q), bz = sz * part_of(e.bk, q), cz = sz * part_of(e.ck, q);
  const float T = (U * az + V * bz) + W * cz;
  const float t = T / det;
  if (!(t >= tmin && t <= tmax)) return false;   // a NaN fails
  h.t = t == 0.0f ? 0.0f : t;                    // -0 is stored as +0
  h.u = U / det, h.v = V / det, h.w = W / det;
  return true;
}

// grid (query blocks, splits, B).  keys != null (splits > 1): one key per (image, split, ray) for k_nearest_merge;
// keys == null: the face, -1 for a ray without a hit in this launch's triangles.
template <typename F>
__global__ __launch_bounds__(kThreads) void k_ray_search(const float *__restrict__ origins,
                                                         const float *__restrict__ directions,
                                                         const float4 *__restrict__ records,
                                                         const int32_t *__restrict__ lengths, int N, int T, int chunk,
                                                         float tmin, float tmax, int32_t *__restrict__ face,
                                                         unsigned long long *__restrict__ keys) {
  constexpr int Q = (int)(sizeof(F) / sizeof(float));
  __shared__ float4 tile[kTriTile * kWnRecWords];
  const int b = (int)blockIdx.z, split = (int)blockIdx.y;
  const int nv = valid_count(lengths, b, N);
  const float4 *rb = records + (size_t)b * T * kWnRecWords;
  const Range run = split_range(split, chunk, T);
  const int i0 = (int)blockIdx.x * (kThreads * Q) + (int)threadIdx.x;

  float ox[Q], oy[Q], oz[Q], dx[Q], dy[Q], dz[Q], sz[Q], best[Q];
  int bi[Q];
  bool live[Q];
  load_queries<Q>(origins + (size_t)b * N * 3, i0, nv, ox, oy, oz);
  load_queries<Q>(directions + (size_t)b * N * 3, i0, nv, dx, dy, dz);
  RayLanes<F> ray;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const Ray r = ray_of(V3{ox[q], oy[q], oz[q]}, V3{dx[q], dy[q], dz[q]}, i0 + q * kThreads < nv);
    set_ray(ray, q, r);
    sz[q] = r.sz;
    live[q] = r.live;
    best[q] = INFINITY;
    bi[q] = -1;
  }

  for (int t0 = run.j0; t0 < run.j1; t0 += kTriTile) {
    const int count = min(kTriTile, run.j1 - t0);
    __syncthreads();
    for (int f = (int)threadIdx.x; f < count * kWnRecWords; f += kThreads)
      tile[f] = rb[(size_t)t0 * kWnRecWords + f];
    __syncthreads();
    for (int j = 0; j < count; ++j) {
      const float4 *r = &tile[j * kWnRecWords];   // one address for the wavefront
      const float4 r0 = r[0];
      const RayEdges<F> e = ray_edges<F>(ray, r0, r[1], r[2]);
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const float u = part_of(e.u, q), v = part_of(e.v, q), w = part_of(e.w, q);
        const float lo = fminf(u, fminf(v, w)), hi = fmaxf(u, fmaxf(v, w));
        // rare: the pair passes the sign test (or holds a NaN); a skipped record (all its edge functions are 0)
        // and a dead ray stay out
        if (__builtin_expect(r0.w != 0.0f && live[q] && !(lo < 0.0f && hi > 0.0f), 0)) {
          RayHit h;
          if (ray_accept(e, q, sz[q], tmin, tmax, h) && h.t < best[q]) {   // strict, faces ascending: the lowest face
            best[q] = h.t;
            bi[q] = t0 + j;
          }
        }
      }
    }
  }

#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = i0 + q * kThreads;
    if (i >= N) continue;
    const bool found = i < nv && bi[q] >= 0;
    if (keys)
      keys[((size_t)b * gridDim.y + split) * N + i] = found ? key_of(best[q], bi[q]) : kNoKey;
    else
      face[(size_t)b * N + i] = found ? bi[q] : -1;
  }
}

// The chosen pair of every ray once more, with the search's own functions -> t, face, bary; +inf / -1 / 0 for a ray
// without a hit.  grid (ceil(N / kThreads), B)
__global__ __launch_bounds__(kThreads) void k_ray_finish(const V3 *__restrict__ origins,
                                                         const V3 *__restrict__ directions,
                                                         const float4 *__restrict__ records,
                                                         const int32_t *__restrict__ lengths, int N, int T, float tmin,
                                                         float tmax, float *__restrict__ t, int32_t *__restrict__ face,
                                                         V3 *__restrict__ bary) {
  const int b = (int)blockIdx.y;
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= N) return;
  const size_t row = (size_t)b * N + i;
  const int f = i < valid_count(lengths, b, N) ? face[row] : -1;
  RayHit h;
  bool hit = false;
  if ((unsigned)f < (unsigned)T) {
    const Ray r = ray_of(origins[row], directions[row], true);
    const float4 *rec = records + ((size_t)b * T + f) * kWnRecWords;
    const float4 r0 = rec[0];
    if (r.live && r0.w != 0.0f) {
      RayLanes<float> ray;
      set_ray(ray, 0, r);
      hit = ray_accept(ray_edges<float>(ray, r0, rec[1], rec[2]), 0, r.sz, tmin, tmax, h);
    }
  }
  t[row] = hit ? h.t : INFINITY;
  face[row] = hit ? f : -1;
  bary[row] = hit ? V3{h.u, h.v, h.w} : V3{0.0f, 0.0f, 0.0f};
}

// g = n / (n . d) of ray i's face, n = (b - a) x (c - a).  False -- a zero gradient -- for a row without a face, a
// face that is not usable, n . d == 0 and a g that is not finite.  nv: the image's valid rays.
__device__ __forceinline__ bool ray_gradient(const V3 *__restrict__ vb, const int32_t *__restrict__ triangles,
                                             const int32_t *__restrict__ fb, const V3 *__restrict__ db, int i, int nv,
                                             int V, int T, V3 &g) {
  if (i >= nv) return false;
  const int f = fb[i];
  if ((unsigned)f >= (unsigned)T) return false;
  int ia, ib, ic;
  if (!usable_triangle(triangles, f, V, ia, ib, ic)) return false;
  const V3 a = vb[ia], p = vb[ib], c = vb[ic], d = db[i];
  const float e0x = p.x - a.x, e0y = p.y - a.y, e0z = p.z - a.z;
  const float e1x = c.x - a.x, e1y = c.y - a.y, e1z = c.z - a.z;
  const float nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
  const float s = nx * d.x + ny * d.y + nz * d.z;
  if (s == 0.0f) return false;
  g = V3{nx / s, ny / s, nz / s};
  return finite3(g);
}

// dorigins[b, i] = -g_i G_i and ddirections[b, i] = -g_i t_i G_i (either may be null), g_i the upstream gradient of
// t_i and G_i ray_gradient's vector; 0 for a ray without a hit.  grid (ceil(N / kThreads), B)
__global__ __launch_bounds__(kThreads) void k_ray_backward_rays(
    const V3 *__restrict__ directions, const V3 *__restrict__ vertices, const int32_t *__restrict__ triangles,
    const int32_t *__restrict__ lengths, int N, int V, int T, const float *__restrict__ t,
    const int32_t *__restrict__ face, const float *__restrict__ g_t, V3 *__restrict__ dorigins,
    V3 *__restrict__ ddirections) {
  const int b = (int)blockIdx.y;
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= N) return;
  const size_t row = (size_t)b * N + i;
  V3 dorigin = {0.0f, 0.0f, 0.0f}, ddirection = dorigin, g;
  if (ray_gradient(vertices + (size_t)b * V, triangles, face + (size_t)b * N, directions + (size_t)b * N, i,
                   valid_count(lengths, b, N), V, T, g)) {
    const float up = -g_t[row], upt = up * t[row];
    dorigin = V3{up * g.x, up * g.y, up * g.z};
    ddirection = V3{upt * g.x, upt * g.y, upt * g.z};
  }
  if (dorigins) dorigins[row] = dorigin;
  if (ddirections) ddirections[row] = ddirection;
}

// dvertices[b, v] = sum over the (ray, corner) entries that name v of g_i bary_ik G_i: order [B, 3N] holds the entries
// 3 i + k grouped by vertex, each group ascending, offsets [B, V + 1].  grid (ceil(V / kPointsPerBlock), B)
__global__ __launch_bounds__(kThreads) void k_ray_backward_vertices(
    const V3 *__restrict__ directions, const V3 *__restrict__ vertices, const int32_t *__restrict__ triangles,
    const int32_t *__restrict__ lengths, int N, int V, int T, const int32_t *__restrict__ face,
    const V3 *__restrict__ bary, const int32_t *__restrict__ order, const int32_t *__restrict__ offsets,
    const float *__restrict__ g_t, V3 *__restrict__ dvertices) {
  const int b = (int)blockIdx.y;
  const int nv = valid_count(lengths, b, N);
  gather_rows(b, V, dvertices, [&](int v, int sub, float &dx, float &dy, float &dz) {
    const int32_t *off = offsets + (size_t)b * (V + 1);
    const int e0 = max(off[v], 0), e1 = min(off[v + 1], 3 * N);
    for (int k = e0 + sub; k < e1; k += kLanesPerPoint) {
      const int e = order[(size_t)b * 3 * N + k];
      if ((unsigned)e >= (unsigned)(3 * N)) continue;
      const int i = e / 3, corner = e - 3 * i;
      V3 g;
      if (!ray_gradient(vertices + (size_t)b * V, triangles, face + (size_t)b * N, directions + (size_t)b * N, i, nv,
                        V, T, g))
        continue;
      const V3 w = bary[(size_t)b * N + i];
      const float s = g_t[(size_t)b * N + i] * (corner == 0 ? w.x : (corner == 1 ? w.y : w.z));
      dx += s * g.x;
      dy += s * g.y;
      dz += s * g.z;
    }
  });
}

// ---- launches ---------------------------------------------------------------------------------------------------
// One kernel, workgroups of kThreads, on stream s -> MR_OK or MR_ELAUNCH.
template <typename Kernel, typename... Args>
int launch(Kernel kernel, dim3 grid, hipStream_t s, Args... args) {
  hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, s, args...);
  return check_launch();
}

// rows of the last pass over the queries (the one that writes the distances): what k_nearest_mean adds per image
inline unsigned partial_rows_of(const Plan &p, int N) {
  return p.splits > 1 ? row_blocks_of(N) : (unsigned)p.query_blocks;
}
inline Layout nearest_layout(const Plan &p, int B, int N) {
  return layout_of(p, B, 0, (size_t)N, partial_rows_of(p, N));
}

// the splits' K keys per query; nothing without a split
inline Layout knn_layout(const Plan &p, int B, int N, int K) { return layout_of(p, B, 0, (size_t)N * K, 0); }

inline Plan tri_plan_of(int B, int N, int T) { return plan_of(B, N, T, kTriTile, kTriWideQueries); }
// triangle to point: the T triangles are the queries, one a lane, and the N points the targets that are split
inline Plan point_plan_of(int B, int N, int T) { return plan_of(B, T, N, kPointTile, 1); }
// both triangle searches, over `rows` queries (the points, or the triangles): the finish pass writes the partial sums
inline Layout tri_layout(const Plan &p, int B, int rows, int T) {
  return layout_of(p, B, align_up((size_t)B * T * kRecWords * sizeof(float4), 256), (size_t)rows, row_blocks_of(rows));
}

// What follows either triangle search: the lowest key of a row's splits -> its face / point, -1 without one
// (k_nearest_merge: every row is a query, the other side's lengths bound the index), the chosen pair once more
// (k_nt_finish) and the mean of the rows' distances: over the image's valid points, or with triangle rows over
// its usable triangles (0 without one or without a valid point).
template <bool kRowsAreTriangles>
int finish_triangle_search(const Plan &p, const Workspace &w, const float *points, const int32_t *lengths,
                           const int32_t *usable, int B, int N, int T, float *sqdist, int32_t *chosen, float *bary,
                           float *total, hipStream_t s) {
  const int R = kRowsAreTriangles ? T : N, O = kRowsAreTriangles ? N : T;
  const int32_t *row_lengths = kRowsAreTriangles ? nullptr : lengths;
  const int32_t *other_lengths = kRowsAreTriangles ? lengths : nullptr;
  int rc = MR_OK;
  if (w.keys)
    rc = launch(k_nearest_merge, rows_grid(R, B), s, w.keys, p.splits, row_lengths, other_lengths, R, O, nullptr,
                chosen, nullptr);
  if (rc == MR_OK)
    rc = launch(k_nt_finish<kRowsAreTriangles>, rows_grid(R, B), s, (const V3 *)points, w.records, lengths, N, T,
                sqdist, chosen, (V3 *)bary, w.partials);
  if (rc == MR_OK && total)
    rc = launch(k_nearest_mean, dim3((unsigned)B), s, w.partials, (int)row_blocks_of(R),
                kRowsAreTriangles ? usable : lengths, other_lengths, R, O, 1.0f, 0, total);
  return rc;
}

}  // namespace

void nearest_plan(int B, int N, int M, int *splits, int *queries_per_lane, int *target_tile, int *workgroup) {
  const Plan p = plan_of(B, N, M);
  *splits = p.splits;
  *queries_per_lane = p.queries_per_lane;
  *target_tile = kTile;
  *workgroup = kThreads;
}

size_t nearest_ws(int B, int N, int M) { return nearest_layout(plan_of(B, N, M), B, N).bytes; }

int launch_nearest_forward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B,
                           int N, int M, float *sqdist, int32_t *idx, float *total, float weight, int accumulate,
                           void *ws, hipStream_t s) {
  const Plan p = plan_of(B, N, M);
  const Workspace w = carve(ws, p, nearest_layout(p, B, N), total != nullptr);
  const auto search = p.queries_per_lane == kWideQueries ? k_nearest<kWideQueries> : k_nearest<1>;
  int rc = launch(search, search_grid(p, B), s, x, y, x_lengths, y_lengths, N, M, p.chunk, sqdist, idx, w.keys,
                  w.keys ? nullptr : w.partials);
  if (rc == MR_OK && w.keys)
    rc = launch(k_nearest_merge, rows_grid(N, B), s, w.keys, p.splits, x_lengths, y_lengths, N, M, sqdist, idx,
                w.partials);
  if (rc == MR_OK && total)
    rc = launch(k_nearest_mean, dim3((unsigned)B), s, w.partials, (int)partial_rows_of(p, N), x_lengths, y_lengths, N,
                M, weight, accumulate, total);
  return rc;
}

int launch_nearest_backward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B,
                            int N, int M, const int32_t *idx_xy, const int32_t *order_xy, const int32_t *offsets_xy,
                            const int32_t *idx_yx, const int32_t *order_yx, const int32_t *offsets_yx,
                            const float *grad_points, const float *grad_images, float x_weight, float y_weight,
                            float *dx, float *dy, hipStream_t s) {
  int rc = MR_OK;
  if (dx)   // the gather half of x -> y and the scatter half of y -> x
    rc = launch(k_nearest_backward, groups_grid(N, B), s, (const V3 *)x, (const V3 *)y, x_lengths, y_lengths, N, M,
                idx_xy, grad_points, x_weight, order_yx, offsets_yx, nullptr, y_weight, grad_images, (V3 *)dx);
  if (rc == MR_OK && dy)   // the gather half of y -> x and the scatter half of x -> y
    rc = launch(k_nearest_backward, groups_grid(M, B), s, (const V3 *)y, (const V3 *)x, y_lengths, x_lengths, M, N,
                idx_yx, nullptr, y_weight, order_xy, offsets_xy, grad_points, x_weight, grad_images, (V3 *)dy);
  return rc;
}

void nearest_triangle_plan(int B, int N, int T, int *splits, int *queries_per_lane, int *triangle_tile,
                           int *workgroup) {
  const Plan p = tri_plan_of(B, N, T);
  *splits = p.splits;
  *queries_per_lane = p.queries_per_lane;
  *triangle_tile = kTriTile;
  *workgroup = kThreads;
}

size_t nearest_triangle_ws(int B, int N, int T) { return tri_layout(tri_plan_of(B, N, T), B, N, T).bytes; }

int launch_nearest_triangle_forward(const float *points, const float *vertices, const int32_t *triangles,
                                    const int32_t *lengths, int B, int N, int V, int T, float *sqdist, int32_t *face,
                                    float *bary, float *total, void *ws, hipStream_t s) {
  const Plan p = tri_plan_of(B, N, T);
  const Workspace w = carve(ws, p, tri_layout(p, B, N, T), total != nullptr);
  int rc = launch(k_nt_setup, rows_grid(T, B), s, (const V3 *)vertices, triangles, V, T, w.records);
  if (rc != MR_OK) return rc;
  const auto search = p.queries_per_lane == kTriWideQueries ? k_nt_search<F2> : k_nt_search<float>;
  rc = launch(search, search_grid(p, B), s, points, w.records, lengths, N, T, p.chunk, face, w.keys);
  if (rc != MR_OK) return rc;
  return finish_triangle_search<false>(p, w, points, lengths, nullptr, B, N, T, sqdist, face, bary, total, s);
}

int launch_nearest_triangle_backward(const float *points, const float *vertices, const int32_t *triangles,
                                     const int32_t *lengths, int B, int N, int V, int T, const int32_t *face,
                                     const float *bary, const int32_t *order, const int32_t *offsets,
                                     const float *grad_points, const float *grad_images, float *dpoints,
                                     float *dvertices, hipStream_t s) {
  int rc = MR_OK;
  if (dpoints)
    rc = launch(k_nt_backward_points, rows_grid(N, B), s, (const V3 *)points, (const V3 *)vertices, triangles, lengths,
                N, V, T, face, (const V3 *)bary, grad_points, grad_images, (V3 *)dpoints);
  if (rc == MR_OK && dvertices)
    rc = launch(k_nt_backward_vertices<false>, groups_grid(V, B), s, (const V3 *)points, (const V3 *)vertices,
                triangles, lengths, N, V, T, face, (const V3 *)bary, order, offsets, grad_points, grad_images, nullptr,
                (V3 *)dvertices);
  return rc;
}

void nearest_point_of_triangle_plan(int B, int N, int T, int *splits, int *points_per_step, int *point_tile,
                                    int *workgroup) {
  *splits = point_plan_of(B, N, T).splits;
  *points_per_step = N >= kPackedFrom ? 2 : 1;
  *point_tile = kPointTile;
  *workgroup = kThreads;
}

size_t nearest_point_of_triangle_ws(int B, int N, int T) { return tri_layout(point_plan_of(B, N, T), B, T, T).bytes; }

int launch_nearest_point_of_triangle_forward(const float *points, const float *vertices, const int32_t *triangles,
                                             const int32_t *lengths, int B, int N, int V, int T, float *sqdist,
                                             int32_t *index, float *bary, float *total, int32_t *usable, void *ws,
                                             hipStream_t s) {
  const Plan p = point_plan_of(B, N, T);
  const Workspace w = carve(ws, p, tri_layout(p, B, T, T), total != nullptr);
  int rc = launch(k_nt_setup, rows_grid(T, B), s, (const V3 *)vertices, triangles, V, T, w.records);
  if (rc != MR_OK) return rc;
  const auto search = N >= kPackedFrom ? k_tp_search<F2> : k_tp_search<float>;
  rc = launch(search, search_grid(p, B), s, points, w.records, lengths, N, T, p.chunk, index, w.keys);
  if (rc == MR_OK && usable) rc = launch(k_tp_usable, dim3(1), s, triangles, V, T, B, usable);   // the mean's divisor
  if (rc != MR_OK) return rc;
  return finish_triangle_search<true>(p, w, points, lengths, usable, B, N, T, sqdist, index, bary, total, s);
}

int launch_nearest_point_of_triangle_backward(const float *points, const float *vertices, const int32_t *triangles,
                                              const int32_t *lengths, int B, int N, int V, int T,
                                              const int32_t *index, const float *bary, const int32_t *corner_order,
                                              const int32_t *corner_offsets, const int32_t *point_order,
                                              const int32_t *point_offsets, const float *grad_triangles,
                                              const float *grad_images, const int32_t *usable, float *dpoints,
                                              float *dvertices, hipStream_t s) {
  int rc = MR_OK;
  if (dpoints)
    rc = launch(k_tp_backward_points, groups_grid(N, B), s, (const V3 *)points, (const V3 *)vertices, triangles,
                lengths, N, V, T, index, (const V3 *)bary, point_order, point_offsets, grad_triangles, grad_images,
                usable, (V3 *)dpoints);
  if (rc == MR_OK && dvertices)
    rc = launch(k_nt_backward_vertices<true>, groups_grid(V, B), s, (const V3 *)points, (const V3 *)vertices, triangles,
                lengths, N, V, T, index, (const V3 *)bary, corner_order, corner_offsets, grad_triangles, grad_images,
                usable, (V3 *)dvertices);
  return rc;
}

// the winding number starts from the triangle search's shape: the same tile, one packed pair of queries a lane
inline Plan wn_plan_of(int B, int N, int T) { return plan_of(B, N, T, kTriTile, kTriWideQueries); }
// the triangle records | the splits' 64-bit partials, one per query (splits > 1)
inline Layout wn_layout(const Plan &p, int B, int N, int T) {
  return layout_of(p, B, align_up((size_t)B * T * kWnRecWords * sizeof(float4), 256), (size_t)N, 0);
}

void winding_number_plan(int B, int N, int T, int *splits, int *queries_per_lane, int *triangle_tile, int *workgroup) {
  const Plan p = wn_plan_of(B, N, T);
  *splits = p.splits;
  *queries_per_lane = p.queries_per_lane;
  *triangle_tile = kTriTile;
  *workgroup = kThreads;
}

int winding_number_max_triangles() { return kWnMaxTriangles; }

size_t winding_number_ws(int B, int N, int T) { return wn_layout(wn_plan_of(B, N, T), B, N, T).bytes; }

int launch_winding_number_forward(const float *points, const float *vertices, const int32_t *triangles,
                                  const int32_t *lengths, int B, int N, int V, int T, float *w, void *ws,
                                  hipStream_t s) {
  const Plan p = wn_plan_of(B, N, T);
  const Workspace space = carve(ws, p, wn_layout(p, B, N, T), false);
  long long *partials = (long long *)space.keys;   // null without a split
  int rc = launch(k_wn_setup<false>, rows_grid(T, B), s, (const V3 *)vertices, triangles, V, T, space.records);
  if (rc != MR_OK) return rc;
  const auto sum = p.queries_per_lane == kTriWideQueries ? k_wn_sum<F2> : k_wn_sum<float>;
  rc = launch(sum, search_grid(p, B), s, points, (const float4 *)space.records, lengths, N, T, p.chunk, w, partials);
  if (rc == MR_OK && partials)
    rc = launch(k_wn_merge, rows_grid(N, B), s, (const long long *)partials, p.splits, lengths, N, w);
  return rc;
}

// ray casting has the winding number's shape and workspace: the corner records | the splits' keys, one per ray
void cast_rays_plan(int B, int N, int T, int *splits, int *queries_per_lane, int *triangle_tile, int *workgroup) {
  winding_number_plan(B, N, T, splits, queries_per_lane, triangle_tile, workgroup);
}

size_t cast_rays_ws(int B, int N, int T) { return winding_number_ws(B, N, T); }

int launch_cast_rays_forward(const float *origins, const float *directions, const float *vertices,
                             const int32_t *triangles, const int32_t *lengths, int B, int N, int V, int T, float t_min,
                             float t_max, float *t, int32_t *face, float *bary, void *ws, hipStream_t s) {
  const Plan p = wn_plan_of(B, N, T);
  const Workspace w = carve(ws, p, wn_layout(p, B, N, T), false);
  int rc = launch(k_wn_setup<true>, rows_grid(T, B), s, (const V3 *)vertices, triangles, V, T, w.records);
  if (rc != MR_OK) return rc;
  const auto search = p.queries_per_lane == kTriWideQueries ? k_ray_search<F2> : k_ray_search<float>;
  rc = launch(search, search_grid(p, B), s, origins, directions, (const float4 *)w.records, lengths, N, T, p.chunk,
              t_min, t_max, face, w.keys);
  if (rc == MR_OK && w.keys)
    rc = launch(k_nearest_merge, rows_grid(N, B), s, w.keys, p.splits, lengths, nullptr, N, T, nullptr, face, nullptr);
  if (rc != MR_OK) return rc;
  return launch(k_ray_finish, rows_grid(N, B), s, (const V3 *)origins, (const V3 *)directions,
                (const float4 *)w.records, lengths, N, T, t_min, t_max, t, face, (V3 *)bary);
}

int launch_cast_rays_backward(const float *directions, const float *vertices, const int32_t *triangles,
                              const int32_t *lengths, int B, int N, int V, int T, const float *t, const int32_t *face,
                              const float *bary, const int32_t *order, const int32_t *offsets, const float *grad_t,
                              float *dorigins, float *ddirections, float *dvertices, hipStream_t s) {
  int rc = MR_OK;
  if (dorigins || ddirections)
    rc = launch(k_ray_backward_rays, rows_grid(N, B), s, (const V3 *)directions, (const V3 *)vertices, triangles,
                lengths, N, V, T, t, face, grad_t, (V3 *)dorigins, (V3 *)ddirections);
  if (rc == MR_OK && dvertices)
    rc = launch(k_ray_backward_vertices, groups_grid(V, B), s, (const V3 *)directions, (const V3 *)vertices, triangles,
                lengths, N, V, T, face, (const V3 *)bary, order, offsets, grad_t, (V3 *)dvertices);
  return rc;
}

int knn_max_k() { return kKnnMaxK; }

void knn_plan(int B, int N, int M, int K, int *splits, int *queries_per_lane, int *list_capacity, int *target_tile,
              int *workgroup) {
  const Plan p = knn_plan_of(B, N, M, K);
  *splits = p.splits;
  *queries_per_lane = p.queries_per_lane;
  *list_capacity = knn_capacity_of(K);
  *target_tile = kTile;
  *workgroup = kThreads;
}

size_t knn_ws(int B, int N, int M, int K) { return knn_layout(knn_plan_of(B, N, M, K), B, N, K).bytes; }

namespace {

template <int C>
int launch_knn_of(const Plan &p, const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths,
                  int B, int N, int M, int K, float *sqdist, int32_t *idx, void *ws, hipStream_t s) {
  constexpr int kWide = knn_wide_queries(C);
  unsigned long long *keys = carve(ws, p, knn_layout(p, B, N, K), false).keys;
  const auto search = (kWide > 1 && p.queries_per_lane == kWide) ? k_knn<C, kWide> : k_knn<C, 1>;
  int rc = launch(search, search_grid(p, B), s, x, y, x_lengths, y_lengths, N, M, K, p.chunk, sqdist, idx, keys);
  if (rc == MR_OK && keys)
    rc = launch(k_knn_merge<C>, rows_grid(N, B), s, keys, p.splits, x_lengths, y_lengths, N, M, K, sqdist, idx);
  return rc;
}

}  // namespace

int launch_knn_forward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B, int N,
                       int M, int K, float *sqdist, int32_t *idx, void *ws, hipStream_t s) {
  const Plan p = knn_plan_of(B, N, M, K);
  switch (knn_capacity_of(K)) {
    case 4: return launch_knn_of<4>(p, x, y, x_lengths, y_lengths, B, N, M, K, sqdist, idx, ws, s);
    case 8: return launch_knn_of<8>(p, x, y, x_lengths, y_lengths, B, N, M, K, sqdist, idx, ws, s);
    case 16: return launch_knn_of<16>(p, x, y, x_lengths, y_lengths, B, N, M, K, sqdist, idx, ws, s);
    default: return launch_knn_of<32>(p, x, y, x_lengths, y_lengths, B, N, M, K, sqdist, idx, ws, s);
  }
}

int launch_knn_backward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B, int N,
                        int M, int K, const float *sqdist, const int32_t *idx, const int32_t *order,
                        const int32_t *offsets, const float *grad, float *dx, float *dy, hipStream_t s) {
  int rc = MR_OK;
  if (dx)
    rc = launch(k_knn_backward<false>, groups_grid(N, B), s, (const V3 *)x, (const V3 *)y, x_lengths, y_lengths, N, M,
                N, K, sqdist, idx, nullptr, nullptr, grad, (V3 *)dx);
  if (rc == MR_OK && dy)
    rc = launch(k_knn_backward<true>, groups_grid(M, B), s, (const V3 *)y, (const V3 *)x, y_lengths, x_lengths, M, N, N,
                K, sqdist, idx, order, offsets, grad, (V3 *)dy);
  return rc;
}

}  // namespace mr
