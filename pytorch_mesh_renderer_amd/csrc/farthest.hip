// Farthest-point sampling of point clouds (mr_farthest_*; INTEGRATION.md, "Farthest-point sampling").
//
// The definition is part of the interface (include/mesh_raster.h) and leaves the kernels no freedom: every valid
// point carries a float32 running distance m (+inf; 0 for a point with a non-finite coordinate), after the selection
// of s every m_i becomes min(m_i, d_i) with d_i = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) in un-fused binary32
// (this file is compiled with -ffp-contract=off), m_s becomes -1, and the next selection is the largest m, the
// lowest index among equals.  That arg-max is ONE unsigned compare of the 64-bit key
//     (bits of m) << 32 | (0xFFFFFFFF - i)           (0 for a point that is selected already, or padding)
// because the bit patterns of the non-negative floats order like the floats.  A NaN d never passes d < m, so a
// non-finite point is never updated and, once selected, moves nobody -- without a branch.
//
// K selections are a chain of K dependent arg-max reductions over the cloud: the work of a step is tiny, its cost is
// the latency of one reduction.  Two routes (A and B here; `route` 1 and 2 of the ABI), chosen by fps_plan_of:
//
//   A  k_fps_resident: one launch, one workgroup per cloud, all K steps.  Every lane holds P points and their m in
//      VGPRs for the whole run (point j of lane t is i = j W + t).  A step: P updates with the lane's best tracked
//      along (m, index, coordinates), a wave reduction of the key in DPP, one LDS slot per wave that carries the
//      winner's coordinates, ONE __syncthreads(); every wave then reads all slots (the two sets alternate by step
//      parity, so a fast wave cannot overwrite what a slow one still reads).  One wavefront: no LDS, no barrier.
//   B  k_fps_step: one launch per step across the chip, m in the workspace.  Launch k reduces the partial keys that
//      the workgroups of launch k - 1 left (every workgroup, redundantly; the partials carry the winner's
//      coordinates), updates its slice against that winner and writes its own partial into the set of parity k.
//      Stream order is the only synchronisation between workgroups: no flags, no polling, no cooperative launch.
//      k_fps_init before (m, and the empty slots of the outputs) and one single-workgroup launch for step K - 1
//      after: K + 1 launches.
//
// Both routes run the same device functions on the same keys, so idx and radius agree bit for bit.
#include <math.h>

#include "mr_internal.h"

namespace mr {

thread_local int g_fps_workgroup = 0, g_fps_points_per_lane = 0;   // mr_debug_set_farthest_shape (0: the plan's)

namespace {

typedef unsigned long long u64;

constexpr int kStepThreads = 256;     // route B: workgroup size
constexpr int kStepWaves = kStepThreads / kWave;
constexpr int kSlicePoints = 2048;    // route B: points of a workgroup's slice (8 a lane) while slices <= kMaxSlices
constexpr int kMaxSlices = 1024;
constexpr int kMaxWaves = 16;

// Route A's launch shapes in ascending capacity W P; the plan takes the first that holds N.  kResidentMaxN: the
// largest cloud the plan gives to route A (profiles/farthest_bench.txt: the measured crossover); a forced route A
// takes every N up to the last shape's capacity.
struct Shape {
  int workgroup, points_per_lane;
};
constexpr Shape kShapes[] = {{64, 4},   {64, 8},    {256, 4},   {256, 8},  {256, 16},
                             {1024, 8}, {1024, 16}, {1024, 20}, {1024, 24}};
constexpr int kShapeCount = (int)(sizeof(kShapes) / sizeof(kShapes[0]));
constexpr int kResidentCapacity = 1024 * 24;
constexpr int kResidentMaxN = kResidentCapacity;

// What a workgroup leaves for the others: its best key and that point's coordinates.  32 bytes.
struct alignas(16) Slot {
  u64 key;
  float x, y, z, pad;
};

struct Plan {
  int route;   // 1: A, 2: B
  int workgroup, points_per_lane, slices;
  int slice;   // route B: points per slice
};

inline bool shape_exists(int workgroup, int points_per_lane) {
  return (workgroup == 64 || workgroup == 256 || workgroup == 1024) &&
         (points_per_lane == 4 || points_per_lane == 8 || points_per_lane == 16 || points_per_lane == 20 ||
          points_per_lane == 24);
}

// route 0: the plan's; 1 / 2 forced.  -> false where a forced route A cannot hold N.
inline bool fps_plan_of(int N, int route, Plan *p) {
  if (route == 0) route = N <= kResidentMaxN ? 1 : 2;
  p->route = route;
  if (route == 1) {
    p->slices = 1;
    p->slice = N;
    if (shape_exists(g_fps_workgroup, g_fps_points_per_lane)) {   // measurement: tools/fps_bench.py
      p->workgroup = g_fps_workgroup;
      p->points_per_lane = g_fps_points_per_lane;
      return (long long)p->workgroup * p->points_per_lane >= N;
    }
    for (int k = 0; k < kShapeCount; ++k) {
      if (kShapes[k].workgroup * kShapes[k].points_per_lane >= N) {
        p->workgroup = kShapes[k].workgroup;
        p->points_per_lane = kShapes[k].points_per_lane;
        return true;
      }
    }
    return false;
  }
  int slices = (N + kSlicePoints - 1) / kSlicePoints;
  if (slices > kMaxSlices) slices = kMaxSlices;
  p->slice = (N + slices - 1) / slices;
  p->slices = (N + p->slice - 1) / p->slice;
  p->workgroup = kStepThreads;
  p->points_per_lane = (p->slice + kStepThreads - 1) / kStepThreads;
  return true;
}

inline size_t m_bytes(int B, int N) { return align_up((size_t)B * N * sizeof(float), 256); }

// ---- device ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int valid_points(const int32_t *__restrict__ lengths, int b, int N) {
  return lengths ? min(max(lengths[b], 0), N) : N;
}

__device__ __forceinline__ int first_point(const int32_t *__restrict__ start_idx, int b, int nv) {
  return start_idx ? min(max(start_idx[b], 0), nv - 1) : 0;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;   // false for NaN
}

__device__ __forceinline__ float sq_distance(float x, float y, float z, float sx, float sy, float sz) {
#pragma clang fp contract(off)
  const float dx = x - sx, dy = y - sy, dz = z - sz;
  return (dx * dx + dy * dy) + dz * dz;
}

// One point's step: m <- min(m, d) (a NaN d changes nothing), -1 for the selected point itself.
__device__ __forceinline__ float updated(float m, float d, bool is_selected) {
  const float lower = d < m ? d : m;
  return is_selected ? -1.0f : lower;
}

__device__ __forceinline__ u64 key_of(float m, int i) {
  return m >= 0.0f ? ((u64)__float_as_uint(m) << 32) | (u64)(0xFFFFFFFFu - (unsigned)i) : 0ull;
}
__device__ __forceinline__ int key_point(u64 key) { return (int)(0xFFFFFFFFu - (unsigned)key); }
__device__ __forceinline__ float key_radius(u64 key) { return __uint_as_float((unsigned)(key >> 32)); }

template <int kCtrl>
__device__ __forceinline__ u64 dpp_max(u64 key) {
  const int lo = (int)(unsigned)key, hi = (int)(unsigned)(key >> 32);
  const unsigned other_lo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, kCtrl, 0xF, 0xF, false);
  const unsigned other_hi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, kCtrl, 0xF, 0xF, false);
  const u64 other = ((u64)other_hi << 32) | other_lo;
  return other > key ? other : key;
}

// The maximum over each row of 16 lanes, in every lane of the row: quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror, row_mirror.
__device__ __forceinline__ u64 row_max(u64 key) {
  key = dpp_max<0xB1>(key);
  key = dpp_max<0x4E>(key);
  key = dpp_max<0x141>(key);
  return dpp_max<0x140>(key);
}

__device__ __forceinline__ u64 read_lane(u64 key, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)key, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(key >> 32), lane);
  return ((u64)hi << 32) | lo;
}

// The maximum over the wavefront, wave-uniform.
__device__ __forceinline__ u64 wave_max(u64 key) {
  key = row_max(key);
  const u64 a = read_lane(key, 0), b = read_lane(key, 16), c = read_lane(key, 32), d = read_lane(key, 48);
  const u64 ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;
}

struct Pick {   // workgroup-uniform
  u64 key;
  float x, y, z;
};

// The largest key of the workgroup and the coordinates that came with it, known to every wave after ONE barrier
// (none with one wavefront).  slots: kMaxWaves entries of LDS that nobody else touches until the barrier after next.
template <int kWaves>
__device__ __forceinline__ Pick pick_best(u64 key, float x, float y, float z, Slot *slots) {
  const u64 best = wave_max(key);
  const int owner = __builtin_ctzll(__ballot(key == best));   // (a key is unique unless it is 0)
  Pick p{best, readlane_f(x, owner), readlane_f(y, owner), readlane_f(z, owner)};
  if constexpr (kWaves > 1) {
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x >> 6;
    if (lane == 0) slots[wave] = Slot{p.key, p.x, p.y, p.z, 0.0f};
    __syncthreads();
    const int mine = lane & (kMaxWaves - 1);
    Slot s{0ull, 0.0f, 0.0f, 0.0f, 0.0f};
    if (mine < kWaves) s = slots[mine];
    u64 all = row_max(s.key);   // every row of 16 lanes holds every slot
    all = read_lane(all, 0);
    const int won = __builtin_ctzll(__ballot(s.key == all));   // a lane of row 0: the slot's number
    p = Pick{all, readlane_f(s.x, won), readlane_f(s.y, won), readlane_f(s.z, won)};
  }
  return p;
}

// Slots k >= min(K, length) of a cloud: idx -1, radius 0.
__device__ __forceinline__ void fill_empty_slots(int32_t *__restrict__ idx, float *__restrict__ radius, int steps,
                                                 int K, int first, int stride) {
  for (int k = steps + first; k < K; k += stride) {
    idx[k] = -1;
    radius[k] = 0.0f;
  }
}

// Route A.  grid (B), W threads.
template <int P, int W>
__global__ __launch_bounds__(W) void k_fps_resident(const float *__restrict__ points,
                                                    const int32_t *__restrict__ lengths,
                                                    const int32_t *__restrict__ start_idx, int N, int K,
                                                    int32_t *__restrict__ idx, float *__restrict__ radius) {
  constexpr int kWaves = W / kWave;
  __shared__ Slot slots[2][kMaxWaves];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int nv = valid_points(lengths, b, N);
  const int steps = min(K, nv);
  int32_t *ib = idx + (size_t)b * K;
  float *rb = radius + (size_t)b * K;
  fill_empty_slots(ib, rb, steps, K, tid, W);
  if (steps == 0) return;   // (the whole workgroup)
  const float *pb = points + (size_t)b * N * 3;

  float px[P], py[P], pz[P], pm[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    // without a branch (one would make the compiler carry the arrays as whole vectors through it): a lane beyond
    // the cloud reads point 0 and is never a candidate
    const int i = j * W + tid;
    const size_t at = 3 * (size_t)(i < nv ? i : 0);
    px[j] = pb[at], py[j] = pb[at + 1], pz[j] = pb[at + 2];
    pm[j] = i < nv ? (finite3(px[j], py[j], pz[j]) ? INFINITY : 0.0f) : -1.0f;
  }

  int s = first_point(start_idx, b, nv);
  float sx = pb[3 * (size_t)s], sy = pb[3 * (size_t)s + 1], sz = pb[3 * (size_t)s + 2];
  float r = INFINITY;
  for (int k = 0;; ++k) {
    if (tid == 0) {
      ib[k] = s;
      rb[k] = r;
    }
    if (k + 1 == steps) break;
    const bool own = tid == (s & (W - 1));   // point s is point s / W (wave-uniform) of lane s % W
    const int js = s / W;
    float bm = -1.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
    int bj = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float m = updated(pm[j], sq_distance(px[j], py[j], pz[j], sx, sy, sz), own && js == j);
      pm[j] = m;
      if (m > bm) {   // ascending index within the lane: the lowest of equals stays
        bm = m, bj = j * W;
        bx = px[j], by = py[j], bz = pz[j];
      }
    }
    const Pick p = pick_best<kWaves>(key_of(bm, bj + tid), bx, by, bz, slots[k & 1]);
    s = key_point(p.key), r = key_radius(p.key);
    sx = p.x, sy = p.y, sz = p.z;
  }
}

// Route B, before the first step: m of every point, and the outputs' empty slots.  grid (blocks, B)
__global__ __launch_bounds__(kStepThreads) void k_fps_init(const float *__restrict__ points,
                                                           const int32_t *__restrict__ lengths, int N, int K,
                                                           float *__restrict__ m, int32_t *__restrict__ idx,
                                                           float *__restrict__ radius) {
  const int b = (int)blockIdx.y;
  const int nv = valid_points(lengths, b, N);
  const int first = (int)blockIdx.x * kStepThreads + (int)threadIdx.x, stride = (int)gridDim.x * kStepThreads;
  fill_empty_slots(idx + (size_t)b * K, radius + (size_t)b * K, min(K, nv), K, first, stride);
  const float *pb = points + (size_t)b * N * 3;
  float *mb = m + (size_t)b * N;
  for (int i = first; i < N; i += stride) {
    float v = -1.0f;
    if (i < nv) v = finite3(pb[3 * (size_t)i], pb[3 * (size_t)i + 1], pb[3 * (size_t)i + 2]) ? INFINITY : 0.0f;
    mb[i] = v;
  }
}

// Route B, step k.  grid (slices, B), or (1, B) with update 0 for the last step.  partials: [2][B][slices].
__global__ __launch_bounds__(kStepThreads) void k_fps_step(const float *__restrict__ points,
                                                           const int32_t *__restrict__ lengths,
                                                           const int32_t *__restrict__ start_idx, int N, int K, int k,
                                                           int slices, int slice, int update, float *__restrict__ m,
                                                           Slot *__restrict__ partials, int32_t *__restrict__ idx,
                                                           float *__restrict__ radius) {
  __shared__ Slot slots[2][kMaxWaves];
  const int b = (int)blockIdx.y, g = (int)blockIdx.x, tid = (int)threadIdx.x, B = (int)gridDim.y;
  const int nv = valid_points(lengths, b, N);
  const int steps = min(K, nv);
  if (k >= steps) return;   // (the whole workgroup)
  const float *pb = points + (size_t)b * N * 3;

  // the selection of step k: the start, or the best of what launch k - 1 left
  int s;
  float sx, sy, sz, r;
  if (k == 0) {
    s = first_point(start_idx, b, nv);
    sx = pb[3 * (size_t)s], sy = pb[3 * (size_t)s + 1], sz = pb[3 * (size_t)s + 2];
    r = INFINITY;
  } else {
    const Slot *left = partials + ((size_t)((k - 1) & 1) * B + b) * slices;
    Slot best{0ull, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int t = tid; t < slices; t += kStepThreads) {
      const Slot other = left[t];
      if (other.key > best.key) best = other;
    }
    const Pick p = pick_best<kStepWaves>(best.key, best.x, best.y, best.z, slots[0]);
    s = key_point(p.key), r = key_radius(p.key);
    sx = p.x, sy = p.y, sz = p.z;
  }
  if (g == 0 && tid == 0) {
    idx[(size_t)b * K + k] = s;
    radius[(size_t)b * K + k] = r;
  }
  if (!update || k + 1 >= steps) return;

  float *mb = m + (size_t)b * N;
  const int i1 = min((g + 1) * slice, nv);   // (slices * slice < 2^31: the plan)
  float bm = -1.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
  int bi = 0;
  for (int i = g * slice + tid; i < i1; i += kStepThreads) {
    const float x = pb[3 * (size_t)i], y = pb[3 * (size_t)i + 1], z = pb[3 * (size_t)i + 2];
    const float v = updated(mb[i], sq_distance(x, y, z, sx, sy, sz), i == s);
    mb[i] = v;
    if (v > bm) {
      bm = v, bi = i;
      bx = x, by = y, bz = z;
    }
  }
  const Pick p = pick_best<kStepWaves>(key_of(bm, bi), bx, by, bz, slots[1]);
  if (tid == 0) partials[((size_t)(k & 1) * B + b) * slices + g] = Slot{p.key, p.x, p.y, p.z, 0.0f};
}

template <int P, int W>
int launch_resident(int B, hipStream_t s, const float *points, const int32_t *lengths, const int32_t *start_idx, int N,
                    int K, int32_t *idx, float *radius) {
  hipLaunchKernelGGL((k_fps_resident<P, W>), dim3((unsigned)B), dim3(W), 0, s, points, lengths, start_idx, N, K, idx,
                     radius);
  return check_launch();
}

template <int W>
int launch_resident_of(int P, int B, hipStream_t s, const float *points, const int32_t *lengths,
                       const int32_t *start_idx, int N, int K, int32_t *idx, float *radius) {
  switch (P) {
    case 4: return launch_resident<4, W>(B, s, points, lengths, start_idx, N, K, idx, radius);
    case 8: return launch_resident<8, W>(B, s, points, lengths, start_idx, N, K, idx, radius);
    case 16: return launch_resident<16, W>(B, s, points, lengths, start_idx, N, K, idx, radius);
    case 20: return launch_resident<20, W>(B, s, points, lengths, start_idx, N, K, idx, radius);
    case 24: return launch_resident<24, W>(B, s, points, lengths, start_idx, N, K, idx, radius);
  }
  return MR_EINVAL;
}

}  // namespace

int farthest_set_shape(int workgroup, int points_per_lane) {
  if (!(workgroup == 0 && points_per_lane == 0) && !shape_exists(workgroup, points_per_lane)) return MR_EINVAL;
  g_fps_workgroup = workgroup;
  g_fps_points_per_lane = points_per_lane;
  return MR_OK;
}

void farthest_plan(int B, int N, int K, int *route, int *workgroup, int *points_per_lane, int *slices) {
  (void)B;   // a step costs the latency of one reduction whatever the batch and however many steps follow
  (void)K;
  Plan p;
  fps_plan_of(N, 0, &p);
  *route = p.route;
  *workgroup = p.workgroup;
  *points_per_lane = p.points_per_lane;
  *slices = p.slices;
}

// the larger of the routes' needs whatever route runs, so that one query serves every forced route: m [B, N] and two
// sets of partials [B, slices]
size_t farthest_ws(int B, int N, int K) {
  (void)K;
  Plan p;
  fps_plan_of(N, 2, &p);
  return m_bytes(B, N) + align_up((size_t)2 * B * p.slices * sizeof(Slot), 256);
}

int launch_farthest_forward(const float *points, const int32_t *lengths, const int32_t *start_idx, int B, int N, int K,
                            int route, int32_t *idx, float *radius, void *ws, hipStream_t s) {
  Plan p;
  if (!fps_plan_of(N, route, &p)) return MR_EINVAL;
  if (p.route == 1) {
    switch (p.workgroup) {
      case 64: return launch_resident_of<64>(p.points_per_lane, B, s, points, lengths, start_idx, N, K, idx, radius);
      case 256: return launch_resident_of<256>(p.points_per_lane, B, s, points, lengths, start_idx, N, K, idx, radius);
      case 1024:
        return launch_resident_of<1024>(p.points_per_lane, B, s, points, lengths, start_idx, N, K, idx, radius);
    }
    return MR_EINVAL;
  }
  float *m = (float *)ws;
  Slot *partials = (Slot *)((char *)ws + m_bytes(B, N));
  const int most = N > K ? N : K;
  int blocks = (most + kStepThreads - 1) / kStepThreads;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(k_fps_init, dim3((unsigned)blocks, (unsigned)B), dim3(kStepThreads), 0, s, points, lengths, N, K, m,
                     idx, radius);
  int rc = check_launch();
  for (int k = 0; k < K && rc == MR_OK; ++k) {
    const int update = k + 1 < K ? 1 : 0;
    hipLaunchKernelGGL(k_fps_step, dim3(update ? (unsigned)p.slices : 1u, (unsigned)B), dim3(kStepThreads), 0, s,
                       points, lengths, start_idx, N, K, k, p.slices, p.slice, update, m, partials, idx, radius);
    rc = check_launch();
  }
  return rc;
}

}  // namespace mr
