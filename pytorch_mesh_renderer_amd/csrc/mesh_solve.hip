// The solve behind Laplacian-preconditioned mesh fitting (mr_laplacian_*; INTEGRATION.md, "Preconditioned
// optimisation"):  A = I + lam L,  L = D - Adj the combinatorial Laplacian of mesh_topology()'s CSR adjacency.
//
//   k_lap_apply     y = A x: one lane per vertex, C channels, the row's neighbours gathered in CSR order and the
//                   row evaluated in float64, rounded once.
//   the solve       Jacobi-preconditioned conjugate gradients, one system per (image, channel), the C channels of an
//                   image in lock-step.  The algorithm and its freeze rules are part of the interface
//                   (include/mesh_raster.h); Sys and sys_start / sys_alpha / sys_beta below are those rules, and
//                   both routes call them on the same reduced scalars.
//
// A CG iteration is a gather over the adjacency and two dot products: bound by the latency of its reductions, not
// by bandwidth.  Two routes (`route` 1 and 2 of the ABI), chosen by plan_of from V alone:
//
//   1  k_cg_resident: one launch, one workgroup per image, every iteration.  x, r, p and the row's diagonal live in
//      registers, P vertices a lane (vertex j of lane t is i = j W + t); p is published through LDS for the gather;
//      the dot products are float64, reduced in DPP within a wave and through one LDS slot per wave.  The workgroup
//      leaves the loop once all its C systems are frozen (a workgroup-uniform branch: the bits cannot change again).
//   2  k_cg_init, then k_cg_direction + k_cg_update per iteration, then k_cg_finish, across the chip.  Every launch
//      leaves per-workgroup partial dot products in the workspace; the next launch sums them in a fixed order in
//      EVERY workgroup (redundantly) and advances the systems' state from them.  p is double-buffered: the gather
//      of k_cg_direction rebuilds a neighbour's new p from z and the OLD p, so it never reads what its own launch
//      writes.  Stream order is the only synchronisation between workgroups: no flags, no polling, no atomics, no
//      cooperative launch.  The number of launches is fixed by the iteration range the caller asks for.
//
// Every in-kernel loop is bounded by max_iterations, a row length or the slice count; every barrier is reached by
// every lane of its workgroup (frozen systems are masked with selects, never branched around).  The order of every
// sum depends on (V, C, route) alone -- not on B and not on which systems still run -- so two runs, a batch and its
// single calls, and a longer run wherever the shorter one had frozen, agree bit for bit.
#include <math.h>

#include "mr_internal.h"

namespace mr {

namespace {

constexpr int kMaxWaves = 16;
constexpr int kStepThreads = 256;   // route 2: workgroup size
constexpr int kStepWaves = kStepThreads / kWave;
constexpr int kMaxSlices = 1024;    // route 2: workgroups per image
constexpr int kRowChunk = 8;        // neighbour indices loaded together (row_sum)

// Route 1's launch shapes in ascending capacity W P; the plan takes the first that holds V.  The last one's p
// occupies 3072 * 4 C bytes of LDS (48 KB at C = 4); 1024 lanes of 3 vertices would hold as much, but at 128 VGPRs a
// lane that shape spills from C = 2 on, and 512 lanes have 256.
struct Shape {
  int workgroup, vertices_per_lane;
};
constexpr Shape kShapes[] = {{64, 2}, {256, 4}, {512, 6}};
constexpr int kShapeCount = (int)(sizeof(kShapes) / sizeof(kShapes[0]));
constexpr int kResidentMaxV = 512 * 6;

struct Plan {
  int route;   // 1 / 2
  int workgroup, vertices_per_lane, slices;
  int slice;   // route 2: vertices per workgroup
};

// route 0: the plan's; 1 / 2 forced.  -> false where a forced route 1 cannot hold V.
inline bool plan_of(int V, int C, int route, Plan *p) {
  (void)C;   // (every shape holds four channels)
  if (route == 0) route = V <= kResidentMaxV ? 1 : 2;
  p->route = route;
  if (route == 1) {
    p->slices = 1;
    p->slice = V;
    for (int k = 0; k < kShapeCount; ++k) {
      if (kShapes[k].workgroup * kShapes[k].vertices_per_lane >= V) {
        p->workgroup = kShapes[k].workgroup;
        p->vertices_per_lane = kShapes[k].vertices_per_lane;
        return true;
      }
    }
    return false;
  }
  const int per_lane = (int)(((long long)V + (long long)kStepThreads * kMaxSlices - 1) / ((long long)kStepThreads * kMaxSlices));
  p->workgroup = kStepThreads;
  p->vertices_per_lane = per_lane;
  p->slice = kStepThreads * per_lane;
  p->slices = (V + p->slice - 1) / p->slice;
  return true;
}

// One system's state.  frozen: 0 running, 1 frozen, 2 frozen as a whole-NaN system (rule 2).
struct alignas(16) Sys {
  double rho, bb, rr;
  int frozen, iters;
};

inline size_t plane_bytes(int B, int V, int C) { return align_up((size_t)B * V * C * sizeof(float), 256); }
inline size_t part_a_bytes(int B, int C, int slices) { return align_up((size_t)B * slices * C * sizeof(double), 256); }
inline size_t part_b_bytes(int B, int C, int slices) { return align_up((size_t)B * slices * 3 * C * sizeof(double), 256); }
inline size_t state_bytes(int B, int C) { return align_up((size_t)B * C * sizeof(Sys), 256); }

// ---- device ---------------------------------------------------------------------------------------------------------
// A value that every lane of the wavefront holds, moved to scalar registers: the systems' state and the reduced dot
// products are the same in every lane, and kept per lane they would cost up to forty VGPRs.
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uniform(double v) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)bits);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(bits >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) < (double)INFINITY; }   // false for NaN

// Before the first iteration: rule 2 (b.b or the initial r.r not finite), then rule 1.
__device__ __forceinline__ Sys sys_start(double bb, double rr, double rz, double tol2) {
  Sys s;
  s.rho = rz, s.bb = bb, s.rr = rr, s.iters = 0;
  s.frozen = uniform(!(finite_d(bb) && finite_d(rr)) ? 2 : (rr <= tol2 * bb ? 1 : 0));
  return s;
}

// After q = A p: alpha, or rule 3 (breakdown: the system keeps the x it has).  A frozen system gets 0.
__device__ __forceinline__ double sys_alpha(Sys &s, double pq) {
  const bool runs = uniform(s.frozen == 0 && pq > 0.0 && finite_d(pq) ? 1 : 0) != 0;
  if (!runs) {
    s.frozen = s.frozen ? s.frozen : 1;
    return 0.0;
  }
  s.iters += 1;
  return uniform(s.rho / pq);
}

// After the update of r: beta, and rule 1.  A frozen system is left as it is and gets 0.
__device__ __forceinline__ double sys_beta(Sys &s, double rr, double rz, double tol2) {
  if (s.frozen) return 0.0;
  const double beta = uniform(rz / s.rho);
  s.rr = rr, s.rho = rz;
  s.frozen = uniform(rr <= tol2 * s.bb ? 1 : 0);
  return beta;
}

__device__ __forceinline__ Sys uniform_sys(const Sys &s) {
  Sys u;
  u.rho = uniform(s.rho), u.bb = uniform(s.bb), u.rr = uniform(s.rr);
  u.frozen = uniform(s.frozen), u.iters = uniform(s.iters);
  return u;
}

__device__ __forceinline__ float sys_residual(const Sys &s) {
  if (s.frozen == 2) return NAN;
  return s.bb == 0.0 ? 0.0f : (float)sqrt(s.rr / s.bb);
}

template <int kCtrl>
__device__ __forceinline__ double dpp_add(double v) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
  const int lo = (int)(unsigned)bits, hi = (int)(unsigned)(bits >> 32);
  const unsigned other_lo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, kCtrl, 0xF, 0xF, false);
  const unsigned other_hi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, kCtrl, 0xF, 0xF, false);
  return v + __longlong_as_double((long long)(((unsigned long long)other_hi << 32) | other_lo));
}

__device__ __forceinline__ double read_lane_d(double v, int lane) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)bits, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(bits >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The sum over the wavefront, wave-uniform: a butterfly within each row of 16 lanes (quad_perm [1,0,3,2],
// quad_perm [2,3,0,1], row_half_mirror, row_mirror; IEEE addition commutes, so every lane of a row holds the same
// bits), then the four rows as (r0 + r1) + (r2 + r3).
__device__ __forceinline__ double wave_sum(double v) {
  v = dpp_add<0xB1>(v);
  v = dpp_add<0x4E>(v);
  v = dpp_add<0x141>(v);
  v = dpp_add<0x140>(v);
  const double a = read_lane_d(v, 0), b = read_lane_d(v, 16), c = read_lane_d(v, 32), d = read_lane_d(v, 48);
  return uniform((a + b) + (c + d));
}

// The N sums over the workgroup, known to every lane after ONE barrier (none with one wavefront).  slots: kMaxWaves * N
// doubles of LDS that nobody else touches until the barrier after next.
template <int kWaves, int N>
__device__ __forceinline__ void group_sum(double (&v)[N], double *slots) {
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = wave_sum(v[n]);
  if constexpr (kWaves > 1) {
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
      for (int n = 0; n < N; ++n) slots[wave * N + n] = v[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) {
      double total = slots[n];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) total += slots[w * N + n];
      v[n] = uniform(total);
    }
  }
}

struct Row {
  int start, deg;
  float inv_diag;   // M^-1 = 1 / fl(1 + lam deg)
};

// Row i of the adjacency, clamped into the arrays whatever the offsets hold.
__device__ __forceinline__ Row row_of(const int32_t *__restrict__ offsets, int i, int nnz, float lam) {
  Row r;
  r.start = min(max(offsets[i], 0), nnz);
  r.deg = min(max(offsets[i + 1], r.start), nnz) - r.start;
  r.inv_diag = 1.0f / fmaf(lam, (float)r.deg, 1.0f);
  return r;
}

__device__ __forceinline__ Row empty_row() { return Row{0, 0, 1.0f}; }

// out = the row's sum of value(j, c) over its neighbours j in CSR order (an index outside [0, V) adds nothing), in
// float64.  A row is a quantity like the dot products: accumulated in float64 and rounded once (row_apply).  In
// float32 the 299-term sum of a hub's row alone put the x of a delta at that hub 6e-6 |b| off at lam = 100 (up to
// 2e-5 with the right-hand side's scale), six times the tolerance; in float64 it is 1e-8.
template <int C, typename Value>
__device__ __forceinline__ void row_sum(const int32_t *__restrict__ nbr, const Row &row, int V, Value value,
                                        double (&out)[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) out[c] = 0.0;
  // kRowChunk indices at a time: their loads are issued together, so a row costs one round trip to the index
  // array and not one per neighbour (the adds keep CSR order; an entry beyond the row adds +0).
  const int end = row.start + row.deg;
  for (int e = row.start; e < end; e += kRowChunk) {
    int j[kRowChunk];
#pragma unroll
    for (int k = 0; k < kRowChunk; ++k) j[k] = e + k < end ? nbr[e + k] : -1;
#pragma unroll
    for (int k = 0; k < kRowChunk; ++k) {
      const bool have = (unsigned)j[k] < (unsigned)V;
      const int at = have ? j[k] : 0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float v = value(at, c);
        out[c] += have ? (double)v : 0.0;
      }
    }
  }
}

// (A v)_i from v_i and the neighbours' sum: (1 + lam deg) v_i - lam sum in float64, rounded once.
__device__ __forceinline__ float row_apply(const Row &row, float lam, float own, double sum) {
  const double diag = fma((double)lam, (double)row.deg, 1.0);
  return (float)fma(-(double)lam, sum, diag * (double)own);
}

// y = A x.  grid (blocks, B)
template <int C>
__global__ __launch_bounds__(kStepThreads) void k_lap_apply(const float *__restrict__ x,
                                                            const int32_t *__restrict__ offsets,
                                                            const int32_t *__restrict__ nbr, int V, int nnz, float lam,
                                                            float *__restrict__ y) {
  const int i = (int)blockIdx.x * kStepThreads + (int)threadIdx.x;
  if (i >= V) return;
  const float *xb = x + (size_t)blockIdx.y * V * C;
  float *yb = y + (size_t)blockIdx.y * V * C;
  const Row row = row_of(offsets, i, nnz, lam);
  double sum[C];
  row_sum<C>(nbr, row, V, [&](int j, int c) { return xb[(size_t)j * C + c]; }, sum);
#pragma unroll
  for (int c = 0; c < C; ++c) yb[(size_t)i * C + c] = row_apply(row, lam, xb[(size_t)i * C + c], sum[c]);
}

// Route 1.  grid (B), W threads.
template <int C, int P, int W>
__global__ __launch_bounds__(W) void k_cg_resident(const float *__restrict__ rhs, const float *__restrict__ x0,
                                                   const int32_t *__restrict__ offsets,
                                                   const int32_t *__restrict__ nbr, int V, int nnz, float lam,
                                                   double tol2, int max_iterations, float *__restrict__ x,
                                                   int32_t *__restrict__ iterations, float *__restrict__ residual) {
  constexpr int kWaves = W / kWave;
  __shared__ float published[W * P * C];
  __shared__ double slots[2][kMaxWaves * 3 * C];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const float *bv = rhs + (size_t)b * V * C;
  const auto in_lds = [&](int j, int c) { return published[j * C + c]; };

  Row row[P];
  float xv[P][C], rv[P][C], pv[P][C];
  double sums[3 * C];
#pragma unroll
  for (int n = 0; n < 3 * C; ++n) sums[n] = 0.0;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int i = j * W + tid;
    row[j] = i < V ? row_of(offsets, i, nnz, lam) : empty_row();
#pragma unroll
    for (int c = 0; c < C; ++c) {
      rv[j][c] = i < V ? bv[(size_t)i * C + c] : 0.0f;
      xv[j][c] = (i < V && x0) ? x0[((size_t)b * V + i) * C + c] : 0.0f;
      sums[c] += (double)rv[j][c] * (double)rv[j][c];
    }
  }
  if (x0) {   // r = b - A x0  (the whole workgroup)
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int i = j * W + tid;
      if (i < V) {
#pragma unroll
        for (int c = 0; c < C; ++c) published[i * C + c] = xv[j][c];
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < P; ++j) {
      double sum[C];
      row_sum<C>(nbr, row[j], V, in_lds, sum);
#pragma unroll
      for (int c = 0; c < C; ++c) rv[j][c] = rv[j][c] - row_apply(row[j], lam, xv[j][c], sum[c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < P; ++j) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      pv[j][c] = rv[j][c] * row[j].inv_diag;
      sums[C + c] += (double)rv[j][c] * (double)rv[j][c];
      sums[2 * C + c] += (double)rv[j][c] * (double)pv[j][c];
    }
  }
  group_sum<kWaves, 3 * C>(sums, slots[0]);
  Sys sys[C];
#pragma unroll
  for (int c = 0; c < C; ++c) sys[c] = sys_start(sums[c], sums[C + c], sums[2 * C + c], tol2);

  for (int it = 0; it < max_iterations; ++it) {
    bool all_frozen = true;
#pragma unroll
    for (int c = 0; c < C; ++c) all_frozen = all_frozen && sys[c].frozen != 0;
    if (all_frozen) break;   // (the whole workgroup: every lane holds the same sys)
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int i = j * W + tid;
      if (i < V) {
#pragma unroll
        for (int c = 0; c < C; ++c) published[i * C + c] = pv[j][c];
      }
    }
    __syncthreads();
    float qv[P][C];
    double pq[C];
#pragma unroll
    for (int c = 0; c < C; ++c) pq[c] = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      double sum[C];
      row_sum<C>(nbr, row[j], V, in_lds, sum);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        qv[j][c] = row_apply(row[j], lam, pv[j][c], sum[c]);
        pq[c] += (double)pv[j][c] * (double)qv[j][c];
      }
    }
    group_sum<kWaves, C>(pq, slots[1]);   // (with more than one wave: a barrier, after which nobody gathers any more)
    float alpha[C];
    bool runs[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      alpha[c] = (float)sys_alpha(sys[c], pq[c]);
      runs[c] = sys[c].frozen == 0;
    }
    double rr[2 * C];
#pragma unroll
    for (int n = 0; n < 2 * C; ++n) rr[n] = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        xv[j][c] = runs[c] ? fmaf(alpha[c], pv[j][c], xv[j][c]) : xv[j][c];
        rv[j][c] = runs[c] ? fmaf(-alpha[c], qv[j][c], rv[j][c]) : rv[j][c];
        const float z = rv[j][c] * row[j].inv_diag;
        rr[c] += (double)rv[j][c] * (double)rv[j][c];
        rr[C + c] += (double)rv[j][c] * (double)z;
      }
    }
    group_sum<kWaves, 2 * C>(rr, slots[0]);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float beta = (float)sys_beta(sys[c], rr[c], rr[C + c], tol2);
#pragma unroll
      for (int j = 0; j < P; ++j) pv[j][c] = runs[c] ? fmaf(beta, pv[j][c], rv[j][c] * row[j].inv_diag) : pv[j][c];
    }
  }

#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int i = j * W + tid;
    if (i < V) {
#pragma unroll
      for (int c = 0; c < C; ++c) x[((size_t)b * V + i) * C + c] = sys[c].frozen == 2 ? NAN : xv[j][c];
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      iterations[b * C + c] = sys[c].iters;
      residual[b * C + c] = sys_residual(sys[c]);
    }
  }
}

// Route 2: what every kernel of it is handed.  Planes are [B, V, C] f32; part_a [B, slices, C] f64 (p.q of
// k_cg_direction), part_b [B, slices, 3 C] f64 ((b.b,) r.r, r.z of k_cg_init / k_cg_update); state_a is written by
// k_cg_direction and read by k_cg_update, state_b the other way round.
struct Stepped {
  const int32_t *offsets, *nbr;
  int V, nnz, slices, slice;
  float lam;
  double tol2;
  float *x, *r, *z, *q;
  double *part_a, *part_b;
  Sys *state_a, *state_b;
};

// The N sums of an image's partials [slices, N] in a fixed order, in every lane.
template <int N>
__device__ __forceinline__ void sum_partials(const double *__restrict__ partials, int slices, double (&out)[N],
                                             double *slots) {
#pragma unroll
  for (int n = 0; n < N; ++n) out[n] = 0.0;
  for (int g = (int)threadIdx.x; g < slices; g += kStepThreads) {
#pragma unroll
    for (int n = 0; n < N; ++n) out[n] += partials[(size_t)g * N + n];
  }
  group_sum<kStepWaves, N>(out, slots);
}

// The systems of image b after the residual partials that k_cg_init (first) or k_cg_update left; -> all frozen.
template <int C>
__device__ __forceinline__ bool after_residual(const Stepped &a, int b, bool first, Sys (&sys)[C], float (&beta)[C],
                                               double *slots) {
  double sums[3 * C];
  sum_partials<3 * C>(a.part_b + (size_t)b * a.slices * 3 * C, a.slices, sums, slots);
  bool all_frozen = true;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (first) {
      sys[c] = sys_start(sums[c], sums[C + c], sums[2 * C + c], a.tol2);
      beta[c] = 0.0f;
    } else {
      sys[c] = uniform_sys(a.state_b[b * C + c]);
      beta[c] = (float)sys_beta(sys[c], sums[C + c], sums[2 * C + c], a.tol2);
    }
    all_frozen = all_frozen && sys[c].frozen != 0;
  }
  return all_frozen;
}

// Route 2, before the first iteration: x = x0 or 0, r = b - A x0, z = r / M, the old p = 0.  grid (slices, B)
template <int C>
__global__ __launch_bounds__(kStepThreads) void k_cg_init(Stepped a, const float *__restrict__ rhs,
                                                          const float *__restrict__ x0, float *__restrict__ p_old) {
  __shared__ double slots[kMaxWaves * 3 * C];
  const int b = (int)blockIdx.y, g = (int)blockIdx.x, tid = (int)threadIdx.x;
  const size_t image = (size_t)b * a.V * C;
  const float *start = x0 ? x0 + image : nullptr;
  double sums[3 * C];
#pragma unroll
  for (int n = 0; n < 3 * C; ++n) sums[n] = 0.0;
  const int i1 = min((g + 1) * a.slice, a.V);
  for (int i = g * a.slice + tid; i < i1; i += kStepThreads) {
    const Row row = row_of(a.offsets, i, a.nnz, a.lam);
    double sum[C];
    if (start) row_sum<C>(a.nbr, row, a.V, [&](int j, int c) { return start[(size_t)j * C + c]; }, sum);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const size_t at = image + (size_t)i * C + c;
      const float rhs_c = rhs[at];
      const float x_c = start ? start[(size_t)i * C + c] : 0.0f;
      const float r_c = start ? rhs_c - row_apply(row, a.lam, x_c, sum[c]) : rhs_c;
      const float z_c = r_c * row.inv_diag;
      a.x[at] = x_c, a.r[at] = r_c, a.z[at] = z_c, p_old[at] = 0.0f;
      sums[c] += (double)rhs_c * (double)rhs_c;
      sums[C + c] += (double)r_c * (double)r_c;
      sums[2 * C + c] += (double)r_c * (double)z_c;
    }
  }
  group_sum<kStepWaves, 3 * C>(sums, slots);
  if (tid == 0) {
#pragma unroll
    for (int n = 0; n < 3 * C; ++n) a.part_b[((size_t)b * a.slices + g) * 3 * C + n] = sums[n];
  }
}

// Route 2, first half of an iteration: beta from the residual partials, p = z + beta p_old (of the own vertices
// into p_new, of the neighbours on the fly), q = A p, the partials of p.q.  grid (slices, B)
template <int C>
__global__ __launch_bounds__(kStepThreads) void k_cg_direction(Stepped a, int first,
                                                               const float *__restrict__ p_old,
                                                               float *__restrict__ p_new) {
  __shared__ double slots[2][kMaxWaves * 3 * C];
  const int b = (int)blockIdx.y, g = (int)blockIdx.x, tid = (int)threadIdx.x;
  Sys sys[C];
  float beta[C];
  const bool all_frozen = after_residual<C>(a, b, first != 0, sys, beta, slots[0]);
  if (g == 0 && tid == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) a.state_a[b * C + c] = sys[c];
  }
  if (all_frozen) return;   // (the whole workgroup)
  const size_t image = (size_t)b * a.V * C;
  const float *zb = a.z + image, *pb = p_old + image;
  const auto direction = [&](int j, int c) { return fmaf(beta[c], pb[(size_t)j * C + c], zb[(size_t)j * C + c]); };
  double pq[C];
#pragma unroll
  for (int c = 0; c < C; ++c) pq[c] = 0.0;
  const int i1 = min((g + 1) * a.slice, a.V);
  for (int i = g * a.slice + tid; i < i1; i += kStepThreads) {
    const Row row = row_of(a.offsets, i, a.nnz, a.lam);
    double sum[C];
    row_sum<C>(a.nbr, row, a.V, direction, sum);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const size_t at = image + (size_t)i * C + c;
      const float p_c = direction(i, c);
      const float q_c = row_apply(row, a.lam, p_c, sum[c]);
      p_new[at] = p_c, a.q[at] = q_c;
      pq[c] += (double)p_c * (double)q_c;
    }
  }
  group_sum<kStepWaves, C>(pq, slots[1]);
  if (tid == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) a.part_a[((size_t)b * a.slices + g) * C + c] = pq[c];
  }
}

// Route 2, second half: alpha from the partials of p.q, x += alpha p, r -= alpha q, z = r / M, the residual
// partials.  grid (slices, B)
template <int C>
__global__ __launch_bounds__(kStepThreads) void k_cg_update(Stepped a, const float *__restrict__ p) {
  __shared__ double slots[2][kMaxWaves * 2 * C];
  const int b = (int)blockIdx.y, g = (int)blockIdx.x, tid = (int)threadIdx.x;
  double pq[C];
  sum_partials<C>(a.part_a + (size_t)b * a.slices * C, a.slices, pq, slots[0]);
  float alpha[C];
  bool runs[C], any = false;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    Sys sys = uniform_sys(a.state_a[b * C + c]);
    alpha[c] = (float)sys_alpha(sys, pq[c]);
    runs[c] = sys.frozen == 0;
    any = any || runs[c];
    if (g == 0 && tid == 0) a.state_b[b * C + c] = sys;
  }
  if (!any) return;   // (the whole workgroup)
  const size_t image = (size_t)b * a.V * C;
  double sums[2 * C];
#pragma unroll
  for (int n = 0; n < 2 * C; ++n) sums[n] = 0.0;
  const int i1 = min((g + 1) * a.slice, a.V);
  for (int i = g * a.slice + tid; i < i1; i += kStepThreads) {
    const Row row = row_of(a.offsets, i, a.nnz, a.lam);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const size_t at = image + (size_t)i * C + c;
      float r_c = a.r[at];
      if (runs[c]) {
        a.x[at] = fmaf(alpha[c], p[at], a.x[at]);
        r_c = fmaf(-alpha[c], a.q[at], r_c);
        a.r[at] = r_c;
        a.z[at] = r_c * row.inv_diag;
      }
      sums[c] += (double)r_c * (double)r_c;
      sums[C + c] += (double)r_c * (double)(r_c * row.inv_diag);
    }
  }
  group_sum<kStepWaves, 2 * C>(sums, slots[1]);
  if (tid == 0) {
    double *out = a.part_b + ((size_t)b * a.slices + g) * 3 * C;
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = 0.0, out[C + c] = sums[c], out[2 * C + c] = sums[C + c];
  }
}

// Route 2, after the last launch of an iteration range: the systems' state from the residual partials.
// all_frozen NULL: the end of the solve -- iterations, residual, and NaN into the x of a rule-2 system; grid
// (slices, B).  Otherwise only all_frozen[b] is written; grid (1, B).
template <int C>
__global__ __launch_bounds__(kStepThreads) void k_cg_finish(Stepped a, int first, int32_t *__restrict__ iterations,
                                                            float *__restrict__ residual,
                                                            int32_t *__restrict__ all_frozen) {
  __shared__ double slots[kMaxWaves * 3 * C];
  const int b = (int)blockIdx.y, g = (int)blockIdx.x, tid = (int)threadIdx.x;
  Sys sys[C];
  float beta[C];
  const bool frozen = after_residual<C>(a, b, first != 0, sys, beta, slots);
  if (all_frozen) {
    if (tid == 0) all_frozen[b] = frozen ? 1 : 0;
    return;
  }
  if (g == 0 && tid == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      iterations[b * C + c] = sys[c].iters;
      residual[b * C + c] = sys_residual(sys[c]);
    }
  }
  const size_t image = (size_t)b * a.V * C;
  const int i1 = min((g + 1) * a.slice, a.V);
  for (int i = g * a.slice + tid; i < i1; i += kStepThreads) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (sys[c].frozen == 2) a.x[image + (size_t)i * C + c] = NAN;
    }
  }
}

template <int C, int P, int W>
int launch_resident(int B, hipStream_t s, const float *rhs, const float *x0, const int32_t *offsets, const int32_t *nbr,
                    int V, int nnz, float lam, double tol2, int max_iterations, float *x, int32_t *iterations,
                    float *residual) {
  hipLaunchKernelGGL((k_cg_resident<C, P, W>), dim3((unsigned)B), dim3(W), 0, s, rhs, x0, offsets, nbr, V, nnz, lam,
                     tol2, max_iterations, x, iterations, residual);
  return check_launch();
}

template <int C>
int solve_of(const Plan &p, const float *rhs, const float *x0, const int32_t *offsets, const int32_t *nbr, int B, int V,
             int nnz, float lam, double tol, int max_iterations, int first_iteration, int iteration_count,
             int32_t *all_frozen, float *x, int32_t *iterations, float *residual, void *ws, hipStream_t s) {
  const double tol2 = tol * tol;
  if (p.route == 1) {
    if (first_iteration != 0) return MR_OK;   // the one launch of iteration 0 ran them all
    switch (p.workgroup) {
      case 64:
        return launch_resident<C, 2, 64>(B, s, rhs, x0, offsets, nbr, V, nnz, lam, tol2, max_iterations, x,
                                         iterations, residual);
      case 256:
        return launch_resident<C, 4, 256>(B, s, rhs, x0, offsets, nbr, V, nnz, lam, tol2, max_iterations, x,
                                          iterations, residual);
      case 512:
        return launch_resident<C, 6, 512>(B, s, rhs, x0, offsets, nbr, V, nnz, lam, tol2, max_iterations, x,
                                           iterations, residual);
    }
    return MR_EINVAL;
  }
  char *at = (char *)ws;
  const auto take = [&](size_t bytes) {
    char *here = at;
    at += bytes;
    return here;
  };
  Stepped a;
  a.offsets = offsets, a.nbr = nbr;
  a.V = V, a.nnz = nnz, a.slices = p.slices, a.slice = p.slice;
  a.lam = lam, a.tol2 = tol2;
  a.x = x;
  a.r = (float *)take(plane_bytes(B, V, C));
  a.z = (float *)take(plane_bytes(B, V, C));
  a.q = (float *)take(plane_bytes(B, V, C));
  float *directions[2] = {(float *)take(plane_bytes(B, V, C)), (float *)take(plane_bytes(B, V, C))};
  a.part_a = (double *)take(part_a_bytes(B, C, p.slices));
  a.part_b = (double *)take(part_b_bytes(B, C, p.slices));
  a.state_a = (Sys *)take(state_bytes(B, C));
  a.state_b = (Sys *)take(state_bytes(B, C));
  const dim3 grid((unsigned)p.slices, (unsigned)B), block(kStepThreads);
  int rc = MR_OK;
  if (first_iteration == 0) {   // iteration `it` reads directions[(it + 1) & 1] and writes directions[it & 1]
    hipLaunchKernelGGL(k_cg_init<C>, grid, block, 0, s, a, rhs, x0, directions[1]);
    rc = check_launch();
  }
  const int end = first_iteration + iteration_count < max_iterations ? first_iteration + iteration_count
                                                                      : max_iterations;
  for (int it = first_iteration; it < end && rc == MR_OK; ++it) {
    hipLaunchKernelGGL(k_cg_direction<C>, grid, block, 0, s, a, it == 0 ? 1 : 0, directions[(it + 1) & 1],
                       directions[it & 1]);
    rc = check_launch();
    if (rc != MR_OK) break;
    hipLaunchKernelGGL(k_cg_update<C>, grid, block, 0, s, a, directions[it & 1]);
    rc = check_launch();
  }
  if (rc != MR_OK) return rc;
  const int first = end == 0 ? 1 : 0;
  if (end >= max_iterations) {
    hipLaunchKernelGGL(k_cg_finish<C>, grid, block, 0, s, a, first, iterations, residual, (int32_t *)nullptr);
    rc = check_launch();
  } else if (all_frozen) {
    hipLaunchKernelGGL(k_cg_finish<C>, dim3(1u, (unsigned)B), block, 0, s, a, first, iterations, residual, all_frozen);
    rc = check_launch();
  }
  return rc;
}

template <int C>
int apply_of(const float *x, const int32_t *offsets, const int32_t *nbr, int B, int V, int nnz, float lam, float *y,
             hipStream_t s) {
  hipLaunchKernelGGL(k_lap_apply<C>, dim3((unsigned)((V + kStepThreads - 1) / kStepThreads), (unsigned)B),
                     dim3(kStepThreads), 0, s, x, offsets, nbr, V, nnz, lam, y);
  return check_launch();
}

}  // namespace

bool laplacian_solve_plan(int V, int C, int route, int *chosen, int *workgroup, int *vertices_per_lane, int *slices) {
  Plan p;
  if (!plan_of(V, C, route, &p)) return false;
  *chosen = p.route;
  *workgroup = p.workgroup;
  *vertices_per_lane = p.vertices_per_lane;
  *slices = p.slices;
  return true;
}

// the stepped route's need whatever route runs, so that one query serves every forced route: five planes [B, V, C]
// (r, z, q and the two p), the two sets of partials and the two sets of states
size_t laplacian_solve_ws(int B, int V, int C) {
  Plan p;
  plan_of(V, C, 2, &p);
  return 5 * plane_bytes(B, V, C) + part_a_bytes(B, C, p.slices) + part_b_bytes(B, C, p.slices) +
         2 * state_bytes(B, C);
}

int launch_laplacian_apply(const float *x, const int32_t *offsets, const int32_t *nbr, int B, int V, int C, int nnz,
                           float lam, float *y, hipStream_t s) {
  switch (C) {
    case 1: return apply_of<1>(x, offsets, nbr, B, V, nnz, lam, y, s);
    case 2: return apply_of<2>(x, offsets, nbr, B, V, nnz, lam, y, s);
    case 3: return apply_of<3>(x, offsets, nbr, B, V, nnz, lam, y, s);
    case 4: return apply_of<4>(x, offsets, nbr, B, V, nnz, lam, y, s);
  }
  return MR_EINVAL;
}

int launch_laplacian_solve(const float *rhs, const float *x0, const int32_t *offsets, const int32_t *nbr, int B, int V,
                           int C, int nnz, float lam, double tol, int max_iterations, int route, int first_iteration,
                           int iteration_count, int32_t *all_frozen, float *x, int32_t *iterations, float *residual,
                           void *ws, hipStream_t s) {
  Plan p;
  if (!plan_of(V, C, route, &p)) return MR_EINVAL;
  switch (C) {
    case 1:
      return solve_of<1>(p, rhs, x0, offsets, nbr, B, V, nnz, lam, tol, max_iterations, first_iteration,
                         iteration_count, all_frozen, x, iterations, residual, ws, s);
    case 2:
      return solve_of<2>(p, rhs, x0, offsets, nbr, B, V, nnz, lam, tol, max_iterations, first_iteration,
                         iteration_count, all_frozen, x, iterations, residual, ws, s);
    case 3:
      return solve_of<3>(p, rhs, x0, offsets, nbr, B, V, nnz, lam, tol, max_iterations, first_iteration,
                         iteration_count, all_frozen, x, iterations, residual, ws, s);
    case 4:
      return solve_of<4>(p, rhs, x0, offsets, nbr, B, V, nnz, lam, tol, max_iterations, first_iteration,
                         iteration_count, all_frozen, x, iterations, residual, ws, s);
  }
  return MR_EINVAL;
}

}  // namespace mr
