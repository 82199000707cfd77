// Mesh regularisers on gfx950: uniform Laplacian, edge length and normal consistency of a deforming mesh
// (mr_mesh_regularizer_forward / _backward; semantics: INTEGRATION.md, "Mesh regularisers").
//
// Per image b, on a topology derived once from the triangles (unique edges, a neighbour CSR, one "flap"
// (a, b, c, d) per manifold edge and the vertex -> (flap, role) inverse of the flaps):
//   lap  = 1/V sum_i |delta_i|,  delta_i = 1/deg_i sum_{j in N(i)} v_j - v_i      (0 for a vertex without neighbours)
//   edge = 1/E sum_e |v_lo - v_hi|          or  1/E sum_e (|v_lo - v_hi| - target)^2
//   nc   = 1/F sum_flaps (1 - cos(n0, n1)), n0 = (b-a) x (c-a), n1 = (d-a) x (b-a) (0 where |n0| or |n1| <= 1e-8)
// Evaluated so that neither cancels in float32: delta_i as 1/deg_i sum_j (v_j - v_i), from differences (nothing is
// lost against |v| far from the origin), and 1 - cos as |n0/|n0| - n1/|n1||^2 / 2 (nothing is lost against 1 across a
// nearly flat edge).  The backward differentiates the same functions (flap_gradient: d(1 - cos) in closed form).
//
// Both directions are per-destination GATHERS like k_vertex_normals (mesh_ops.hip): eight lanes own one
// (image, vertex), walk its lists eight entries a trip and meet in a fixed butterfly, so every output is written
// exactly once, nothing is zero-filled, and there are no atomics: the results are bitwise reproducible in either
// deterministic mode.  The forward walks a vertex's neighbour list ONCE for delta_i and for its share of the edge
// term (an edge is counted at its lower endpoint); the flaps take a second range of the same grid, one lane each.
// The three per-image scalars are reduced as k_sh_backward reduces dsh: a workgroup stays inside one image
// (grid = (blocks, B)), sums over the wavefront and LDS into one workspace row, and a second small launch adds an
// image's rows in a fixed order.  The backward needs no reduction: one launch.
#include "mr_internal.h"

namespace mr {
namespace {

constexpr int kThreads = 256;          // 4 wavefronts
constexpr int kLanesPerVertex = 8;     // as k_vertex_normals: valence ~6, a second trip beyond 8
constexpr int kVerticesPerBlock = kThreads / kLanesPerVertex;
constexpr float kNormalFloor = 1e-8f;  // a flap with |n0| or |n1| at or below this has value 0 and gradient 0
constexpr int kLap = 1, kEdge = 2, kNc = 4;
static_assert(kThreads == 4 * kWave, "block_sum3 sums four wavefronts");

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator*(float k, V3 a) { return {k * a.x, k * a.y, k * a.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

__device__ __forceinline__ V3 sum_over_vertex_lanes(V3 s) {
#pragma unroll
  for (int m = 1; m < kLanesPerVertex; m <<= 1) {
    s.x += __shfl_xor(s.x, m, kLanesPerVertex);
    s.y += __shfl_xor(s.y, m, kLanesPerVertex);
    s.z += __shfl_xor(s.z, m, kLanesPerVertex);
  }
  return s;
}

// The sum of v over the wavefront, the same on every lane: after each butterfly step the two partners hold the
// same (commuted) sum, so the order is fixed.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// The workgroup's sums of (a, b, c), returned on thread 0.  Every thread of the workgroup calls it.
__device__ __forceinline__ void block_sum3(float &a, float &b, float &c) {
  __shared__ float part[kThreads / kWave][3];
  a = wave_sum(a);
  b = wave_sum(b);
  c = wave_sum(c);
  const int wave = (int)threadIdx.x / kWave;
  if (lane_id() == 0) {
    part[wave][0] = a;
    part[wave][1] = b;
    part[wave][2] = c;
  }
  __syncthreads();
  a = (part[0][0] + part[1][0]) + (part[2][0] + part[3][0]);
  b = (part[0][1] + part[1][1]) + (part[2][1] + part[3][1]);
  c = (part[0][2] + part[1][2]) + (part[2][2] + part[3][2]);
}

struct Flap {
  int a, b, c, d;
  bool ok;
};
__device__ __forceinline__ Flap load_flap(const int32_t *__restrict__ flaps, int f, int V) {
  Flap q;
  q.a = flaps[4 * f];
  q.b = flaps[4 * f + 1];
  q.c = flaps[4 * f + 2];
  q.d = flaps[4 * f + 3];
  q.ok = (unsigned)q.a < (unsigned)V && (unsigned)q.b < (unsigned)V && (unsigned)q.c < (unsigned)V &&
         (unsigned)q.d < (unsigned)V;
  return q;
}

// ---- forward ----------------------------------------------------------------------------------------------------
// Blocks [0, vertex_blocks) of an image: kVerticesPerBlock vertices each, eight lanes a vertex.  Blocks
// [vertex_blocks, gridDim.x): kThreads flaps each, one lane a flap.  Every block writes one row (lap, edge, nc).
__global__ __launch_bounds__(kThreads) void k_mesh_reg_forward(
    const V3 *__restrict__ vertices, const int32_t *__restrict__ nbr_offsets, const int32_t *__restrict__ nbr,
    const int32_t *__restrict__ flaps, int V, int E, int F, int terms, int use_target, float target,
    int vertex_blocks, V3 *__restrict__ unit_dirs, float *__restrict__ rows) {
  const int b = (int)blockIdx.y;
  const V3 *vb = vertices + (size_t)b * V;
  float lap = 0.0f, edge = 0.0f, nc = 0.0f;
  if ((int)blockIdx.x < vertex_blocks) {
    const int v = (int)blockIdx.x * kVerticesPerBlock + (int)threadIdx.x / kLanesPerVertex;
    const int sub = (int)threadIdx.x % kLanesPerVertex;
    const bool have = v < V;   // (whole groups of eight: the butterfly below stays inside one)
    int e0 = 0, e1 = 0;
    V3 vi{0.f, 0.f, 0.f};
    if (have) {
      e0 = max(nbr_offsets[v], 0);
      e1 = min(nbr_offsets[v + 1], 2 * E);
      vi = vb[v];
    }
    V3 s{0.f, 0.f, 0.f};
    for (int i = e0 + sub; i < e1; i += kLanesPerVertex) {
      const int j = nbr[i];
      if ((unsigned)j >= (unsigned)V) continue;
      const V3 d = vb[j] - vi;
      s = s + d;   // differences, not positions: delta_i does not cancel against |v| far from the origin
      if ((terms & kEdge) && j > v) {   // the edge (v, j) is counted here, at its lower endpoint
        const float len = sqrtf(dot(d, d));
        edge += use_target ? (len - target) * (len - target) : len;
      }
    }
    if (terms & kLap) {
      s = sum_over_vertex_lanes(s);
      if (have && sub == 0) {
        V3 u{0.f, 0.f, 0.f};
        const int deg = e1 - e0;
        if (deg > 0) {
          const float inv = 1.0f / (float)deg;
          const V3 delta = inv * s;
          const float len = sqrtf(dot(delta, delta));
          if (len > 0.0f) {
            lap = len;
            u = (1.0f / len) * delta;
          }
        }
        unit_dirs[(size_t)b * V + v] = u;
      }
    }
  } else if (terms & kNc) {
    const int f = ((int)blockIdx.x - vertex_blocks) * kThreads + (int)threadIdx.x;
    if (f < F) {
      const Flap q = load_flap(flaps, f, V);
      if (q.ok) {
        const V3 pa = vb[q.a];
        const V3 p = vb[q.b] - pa, qc = vb[q.c] - pa, r = vb[q.d] - pa;
        const V3 n0 = cross(p, qc), n1 = cross(r, p);
        const float l0 = sqrtf(dot(n0, n0)), l1 = sqrtf(dot(n1, n1));
        if (l0 > kNormalFloor && l1 > kNormalFloor) {
          // 1 - cos as |h0 - h1|^2 / 2 on the unit normals: no cancellation against 1 on a nearly flat flap
          const V3 w = (1.0f / l0) * n0 - (1.0f / l1) * n1;
          nc = 0.5f * dot(w, w);
        }
      }
    }
  }
  block_sum3(lap, edge, nc);
  if (threadIdx.x == 0) {
    float *row = rows + ((size_t)b * gridDim.x + blockIdx.x) * 3;
    row[0] = lap;
    row[1] = edge;
    row[2] = nc;
  }
}

// terms[b] = the sums of image b's `count` workspace rows in a fixed order, over V, E and F (one workgroup per image)
__global__ __launch_bounds__(kThreads) void k_mesh_reg_sum_rows(const float *__restrict__ rows, int count, int V,
                                                                int E, int F, float *__restrict__ out) {
  const int b = (int)blockIdx.x;
  const float *img = rows + (size_t)b * count * 3;
  float lap = 0.0f, edge = 0.0f, nc = 0.0f;
  for (int r = (int)threadIdx.x; r < count; r += kThreads) {
    lap += img[3 * r];
    edge += img[3 * r + 1];
    nc += img[3 * r + 2];
  }
  block_sum3(lap, edge, nc);
  if (threadIdx.x == 0) {
    out[3 * b] = lap / (float)V;
    out[3 * b + 1] = E > 0 ? edge / (float)E : 0.0f;
    out[3 * b + 2] = F > 0 ? nc / (float)F : 0.0f;
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------
// d(1 - cos(n0, n1)) / d(the flap's vertex in `role`: 0 a, 1 b, 2 c, 3 d).  With p = b-a, q = c-a, r = d-a,
// n0 = p x q, n1 = r x p, C = n0.n1 / (|n0| |n1|):
//   dC/dn0 = (n1/|n1| - C n0/|n0|) / |n0| = g0,   dC/dn1 = (n0/|n0| - C n1/|n1|) / |n1| = g1
//   dC/dp = q x g0 + g1 x r,   dC/dq = g0 x p,   dC/dr = p x g1,   dC/da = -(the three)
__device__ __forceinline__ V3 flap_gradient(V3 pa, V3 pb, V3 pc, V3 pd, int role) {
  const V3 p = pb - pa, q = pc - pa, r = pd - pa;
  const V3 n0 = cross(p, q), n1 = cross(r, p);
  const float l0 = sqrtf(dot(n0, n0)), l1 = sqrtf(dot(n1, n1));
  if (!(l0 > kNormalFloor && l1 > kNormalFloor)) return {0.f, 0.f, 0.f};
  const float i0 = 1.0f / l0, i1 = 1.0f / l1;
  const V3 h0 = i0 * n0, h1 = i1 * n1;
  const float C = dot(h0, h1);
  const V3 g0 = i0 * (h1 - C * h0), g1 = i1 * (h0 - C * h1);
  const V3 dp = cross(q, g0) + cross(g1, r), dq = cross(g0, p), dr = cross(p, g1);
  V3 dC;
  if (role == 0) dC = -1.0f * (dp + dq + dr);
  else if (role == 1) dC = dp;
  else if (role == 2) dC = dq;
  else dC = dr;
  return -1.0f * dC;
}

__global__ __launch_bounds__(kThreads) void k_mesh_reg_backward(
    const float *__restrict__ dterms, const V3 *__restrict__ vertices, const V3 *__restrict__ unit_dirs,
    const int32_t *__restrict__ nbr_offsets, const int32_t *__restrict__ nbr, const int32_t *__restrict__ flaps,
    const int32_t *__restrict__ role_offsets, const int32_t *__restrict__ roles, int V, int E, int F, int terms,
    int use_target, float target, V3 *__restrict__ dvertices) {
  const int b = (int)blockIdx.y;
  const int v = (int)blockIdx.x * kVerticesPerBlock + (int)threadIdx.x / kLanesPerVertex;
  const int sub = (int)threadIdx.x % kLanesPerVertex;
  const bool have = v < V;
  const V3 *vb = vertices + (size_t)b * V;
  const float *g = dterms + 3 * b;   // b = blockIdx.y: wave-uniform, scalar loads
  V3 d{0.f, 0.f, 0.f};
  if (have && (terms & (kLap | kEdge))) {
    const V3 *ub = unit_dirs + (size_t)b * V;
    const float glap = (terms & kLap) ? g[0] / (float)V : 0.0f;
    const float gedge = ((terms & kEdge) && E > 0) ? g[1] / (float)E : 0.0f;
    const V3 vk = vb[v];
    const int e0 = max(nbr_offsets[v], 0), e1 = min(nbr_offsets[v + 1], 2 * E);
    V3 dl{0.f, 0.f, 0.f}, de{0.f, 0.f, 0.f};
    for (int i = e0 + sub; i < e1; i += kLanesPerVertex) {
      const int j = nbr[i];
      if ((unsigned)j >= (unsigned)V) continue;
      if (terms & kLap) {   // sum_{i in N(k)} u_i / deg_i
        const int deg = min(nbr_offsets[j + 1], 2 * E) - max(nbr_offsets[j], 0);
        if (deg > 0) dl = dl + (1.0f / (float)deg) * ub[j];
      }
      if (terms & kEdge) {
        const V3 w = vk - vb[j];
        const float len = sqrtf(dot(w, w));
        if (len > 0.0f) de = de + ((use_target ? 2.0f * (len - target) : 1.0f) / len) * w;
      }
    }
    if ((terms & kLap) && sub == 0) dl = dl - ub[v];
    d = glap * dl + gedge * de;
  }
  if (have && (terms & kNc) && F > 0) {
    const float gnc = g[2] / (float)F;
    const int r0 = max(role_offsets[v], 0), r1 = min(role_offsets[v + 1], 4 * F);
    V3 dn{0.f, 0.f, 0.f};
    for (int i = r0 + sub; i < r1; i += kLanesPerVertex) {
      const int entry = roles[i];
      if ((unsigned)entry >= 4u * (unsigned)F) continue;
      const Flap q = load_flap(flaps, entry >> 2, V);
      if (!q.ok) continue;
      dn = dn + flap_gradient(vb[q.a], vb[q.b], vb[q.c], vb[q.d], entry & 3);
    }
    d = d + gnc * dn;
  }
  d = sum_over_vertex_lanes(d);
  if (have && sub == 0) dvertices[(size_t)b * V + v] = d;
}

inline unsigned vertex_blocks_of(int V) { return (unsigned)((V + kVerticesPerBlock - 1) / kVerticesPerBlock); }
inline unsigned flap_blocks_of(int F) { return (unsigned)((F + kThreads - 1) / kThreads); }

}  // namespace

// rows for every block the forward can launch (all three terms), whichever terms a call asks for
size_t mesh_regularizer_ws(int B, int V, int F) {
  return align_up((size_t)B * (vertex_blocks_of(V) + flap_blocks_of(F)) * 3 * sizeof(float), 256);
}

int launch_mesh_regularizer_forward(const float *vertices, const int32_t *nbr_offsets, const int32_t *nbr,
                                    const int32_t *flaps, int B, int V, int E, int F, int terms, int use_target,
                                    float target, float *unit_dirs, float *out_terms, void *ws, hipStream_t s) {
  const unsigned vblocks = (terms & (kLap | kEdge)) ? vertex_blocks_of(V) : 0u;
  const unsigned fblocks = (terms & kNc) ? flap_blocks_of(F) : 0u;
  const unsigned blocks = vblocks + fblocks;
  float *rows = (float *)ws;
  if (blocks > 0) {
    hipLaunchKernelGGL(k_mesh_reg_forward, dim3(blocks, (unsigned)B), dim3(kThreads), 0, s, (const V3 *)vertices,
                       nbr_offsets, nbr, flaps, V, E, F, terms, use_target, target, (int)vblocks, (V3 *)unit_dirs,
                       rows);
    const int rc = check_launch();
    if (rc != MR_OK) return rc;
  }
  hipLaunchKernelGGL(k_mesh_reg_sum_rows, dim3((unsigned)B), dim3(kThreads), 0, s, (const float *)rows, (int)blocks,
                     V, E, F, out_terms);
  return check_launch();
}

int launch_mesh_regularizer_backward(const float *dterms, const float *vertices, const float *unit_dirs,
                                     const int32_t *nbr_offsets, const int32_t *nbr, const int32_t *flaps,
                                     const int32_t *role_offsets, const int32_t *roles, int B, int V, int E, int F,
                                     int terms, int use_target, float target, float *dvertices, hipStream_t s) {
  hipLaunchKernelGGL(k_mesh_reg_backward, dim3(vertex_blocks_of(V), (unsigned)B), dim3(kThreads), 0, s, dterms,
                     (const V3 *)vertices, (const V3 *)unit_dirs, nbr_offsets, nbr, flaps, role_offsets, roles, V, E,
                     F, terms, use_target, target, (V3 *)dvertices);
  return check_launch();
}

}  // namespace mr
