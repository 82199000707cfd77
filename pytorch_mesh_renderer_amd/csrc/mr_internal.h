// Shared device helpers and launch plumbing for the gfx950 rasterizer kernels.
// Everything here is CDNA4-only: wave64, __builtin_amdgcn_* intrinsics.
#pragma once

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mesh_raster.h"

namespace mr {

constexpr int kWave = 64;       // gfx950 wavefront
constexpr int kXcds = 8;        // MI355X: 8 XCDs, each with a private L2

// Per-(image, triangle) setup record produced by k_setup and consumed by the
// raster kernel through wave-uniform (scalar) loads.  64 bytes, 64-B aligned.
//   a = (m0 m1 m2 m3)  b = (m4 m5 m6 m7)  c = (m8 z0 z1 z2)  d = (w0 w1 w2 -)
// m[] is the sign-corrected adjugate of [[x],[y],[w]] (rows = edge functions).
struct alignas(64) TriRec {
  float4 a, b, c, d;
};

// Per-(image, triangle) bbox record, 16 bytes: pixel bbox [l, r) x [bot, top) packed as 4 x u16
// (an empty / culled triangle is all zeros so that no region ever selects it) and a lower bound
// of the depth values the triangle can produce (-inf when none is proven: raster_forward.hip).
struct alignas(16) TriBox {
  unsigned lr, bt;
  float zlo;
  unsigned pad;
};

__device__ __forceinline__ uint2 pack_bbox(int l, int r, int bot, int top) {
  return make_uint2((unsigned)l | ((unsigned)r << 16), (unsigned)bot | ((unsigned)top << 16));
}

__device__ __forceinline__ int lane_id() {
  return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

__device__ __forceinline__ float readlane_f(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// Remap the hardware block id so that each XCD (blocks b, b+8, b+16, ... land
// on the same XCD under round-robin dispatch) owns one CONTIGUOUS range of the
// logical work list.  Placement only affects speed (which L2 holds which
// image's triangle records), never correctness.  Returns -1 for padding blocks.
__device__ __forceinline__ int xcd_contiguous_block(int hw_block, int n_logical, int per_xcd) {
  const int logical = (hw_block % kXcds) * per_xcd + hw_block / kXcds;
  return logical < n_logical ? logical : -1;
}

// ---- host side -------------------------------------------------------------
extern thread_local int g_last_hip_error;

inline int check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    g_last_hip_error = (int)e;
    return MR_ELAUNCH;
  }
  return MR_OK;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Zero-fill as a KERNEL, never hipMemsetAsync.  Round 5: a memset NODE of a captured HIP graph replayed after eager work
// had run on the same device wrote another value than the one captured (ROCm 7.2: the 8-byte empty-block map came out as
// 0xC6 bytes on the second replay, tests/test_render_gpu.py::test_capture_step_replays_the_references_loop); kernel
// nodes carry their arguments by value.  Any alignment, any size; 16-byte stores over the aligned body.
static __global__ __launch_bounds__(256) void k_zero_bytes(unsigned char *__restrict__ p, size_t head, size_t n16, size_t tail) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  uint4 *body = (uint4 *)(p + head);
  for (size_t k = i; k < n16; k += (size_t)gridDim.x * 256) body[k] = make_uint4(0u, 0u, 0u, 0u);
  if (i < head) p[i] = 0;
  if (i < tail) p[head + n16 * 16 + i] = 0;
}
inline hipError_t zero_async(void *ptr, size_t bytes, hipStream_t s) {
  if (bytes == 0 || ptr == nullptr) return hipSuccess;
  unsigned char *p = (unsigned char *)ptr;
  size_t head = (size_t)((16 - ((uintptr_t)p & 15)) & 15);
  if (head > bytes) head = bytes;
  const size_t n16 = (bytes - head) / 16, tail = bytes - head - n16 * 16;
  size_t blocks = (n16 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_zero_bytes, dim3((unsigned)blocks), dim3(256), 0, s, p, head, n16, tail);
  return hipPeekAtLastError();
}

// mr_debug_last_accumulate_kernel (mesh_raster_debug.h): the functor of the most recent per-triangle accumulation
// pass launched by ANY thread of the process (autograd launches backward passes on a thread of its own), as the
// compiler spells it -- e.g. "... [Fn = mr::ShadeFoldLaneFn<1, true>]".  The parity tests read it to make sure the
// specialised kernel they mean to pin to the reference is the one that ran.  One relaxed pointer store per launch.
extern const char *volatile g_last_accumulate_kernel;
// mr_debug_set_lanes_rows / mr_debug_last_lanes_rows (mesh_raster_debug.h): the calling thread's forced strip height
// of k_accumulate_lanes (0: automatic, the default) and the height the last such launch of any thread used.
extern thread_local int g_lanes_rows;
extern volatile int g_last_lanes_rows;

// mr_time_next_kernel (mesh_raster.h): per-thread, one-shot pairs of HIP events recorded on the
// launch stream immediately around one named kernel.  A caller arms a pair, the next launch of
// that kernel ON THE ARMING THREAD consumes it; nothing is recorded otherwise.
struct KernelTimerSlot {
  hipEvent_t start = nullptr, stop = nullptr;
};
extern thread_local KernelTimerSlot g_kernel_timers[MR_TIMER_COUNT];

class KernelTimer {
 public:
  KernelTimer(int which, hipStream_t s) : stream_(s) {
    KernelTimerSlot &slot = g_kernel_timers[which];
    stop_ = slot.stop;
    if (slot.start) (void)hipEventRecord(slot.start, s);
    slot = KernelTimerSlot{};
  }
  ~KernelTimer() {
    if (stop_) (void)hipEventRecord(stop_, stream_);
  }
  KernelTimer(const KernelTimer &) = delete;
  KernelTimer &operator=(const KernelTimer &) = delete;

 private:
  hipStream_t stream_;
  hipEvent_t stop_;
};

// Host launchers (one per .hip file)
int launch_raster_forward(const float *clip, const int32_t *tris, int B, int V, int T, int W,
                          int H, int32_t *ids, float *bary, float *z, void *ws, hipStream_t s);
size_t raster_forward_ws(int B, int V, int T, int W, int H);
int launch_raster_backward(const float *dbary, const float *clip, const int32_t *tris,
                           const int32_t *ids, const float *bary, int B, int V, int T, int W,
                           int H, float *dclip, void *ws, hipStream_t s);
size_t raster_backward_ws(int B, int V, int T, int W, int H);
int launch_interp_forward(const int32_t *ids, const float *bary, const float *attrs,
                          const int32_t *tris, const float *bg, int B, int V, int T, int W,
                          int H, int A, float *out, hipStream_t s);
int launch_interp_backward(const float *dout, const int32_t *ids, const float *bary,
                           const float *attrs, const int32_t *tris, const float *bg, int B,
                           int V, int T, int W, int H, int A, float *dattrs, float *dbary,
                           void *ws, hipStream_t s);
size_t interp_backward_ws(int B, int V, int T, int W, int H, int A);
int shade_max_lights();
int shade_light_gradient_max_lights();
int launch_shade_forward(const int32_t *ids, const float *bary, const float *normals,
                         const float *positions, const float *diffuse, const int32_t *tris,
                         const float *light_pos, const float *light_col, const float *ambient,
                         int B, int V, int T, int W, int H, int L, float *rgba, void *ws,
                         hipStream_t s);
size_t shade_forward_ws(int B, int V, int T, int W, int H);
size_t shade_backward_ws(int B, int V, int T, int W, int H);
int launch_shade_backward(const float *drgba, const uint8_t *signs, const float *sign_upstream,
                          const int32_t *ids, const float *bary,
                          const float *clip, const float *normals, const float *positions,
                          const float *diffuse, const int32_t *tris, const float *light_pos,
                          const float *light_col, const float *ambient, int B, int V, int T, int W,
                          int H, int L, float *dclip, float *dnormals, float *dpositions,
                          float *ddiffuse, float *light_grads, const void *corner_records,
                          const int32_t *vertex_offsets, const int32_t *vertex_entries,
                          const float *transforms, int gbuffer_flags, void *prepared, const uint8_t *empty_regions, void *ws,
                          hipStream_t s);
size_t shade_backward_prepared_bytes(int B, int T);

int interp_raster_max_attrs();
size_t interp_raster_backward_ws(int B, int V, int T, int W, int H, int A);
size_t interp_records_bytes(int B, int T, int A);
int launch_interp_forward_records(const int32_t *ids, const float *bary, const float *attrs, const int32_t *tris,
                                  const float *bg, int B, int V, int T, int W, int H, int A, float *out,
                                  void *records, hipStream_t s);
int launch_interp_raster_backward(const float *dout, const int32_t *ids, const float *bary, const float *clip,
                                  const float *attrs, const int32_t *tris, const float *bg,
                                  const int32_t *offsets, const int32_t *entries, const void *corner_records,
                                  int B, int V, int T, int W, int H, int A, float *dattrs, float *dclip,
                                  int gbuffer_flags, void *ws, hipStream_t s);
int launch_vertex_transform(const float *vertices, const float *transforms, int B, int V, float *clip,
                            hipStream_t s);
int launch_attr_records(const float *attrs, const int32_t *tris, int B, int V, int T, int A, void *records, hipStream_t s);
int launch_rasterize_interpolate_forward(const float *clip, const float *attrs, const int32_t *tris, const float *background,
                                         int B, int V, int T, int W, int H, int A, int32_t *ids, float *bary, float *z,
                                         float *out, void *records, void *ws, hipStream_t s);
int launch_render_forward(const float *vertices, const float *transforms, const float *normals,
                          const float *diffuse, const int32_t *tris, const float *light_pos,
                          const float *light_col, const float *ambient, int B, int V, int T, int W, int H,
                          int L, float *clip, int32_t *ids, float *bary, float *z, int want_z, float *rgba,
                          uint8_t *rgba_u8, void *corner_records, void *backward_prepared, uint8_t *empty_regions, void *ws,
                          hipStream_t s);
// ... and mean|rgba - target| (loss, sign codes) out of the same pass; partials: render_forward_l1_partials() floats
size_t render_forward_l1_partials(int B, int W, int H);
int launch_render_forward_l1(const float *vertices, const float *transforms, const float *normals,
                             const float *diffuse, const int32_t *tris, const float *light_pos,
                             const float *light_col, const float *ambient, int B, int V, int T, int W, int H,
                             int L, float *clip, int32_t *ids, float *bary, float *z, int want_z, float *rgba,
                             uint8_t *rgba_u8, void *corner_records, void *backward_prepared, uint8_t *empty_regions, void *ws,
                             const float *target, const uint8_t *target_empty, float *loss, uint8_t *signs, float *partials,
                             hipStream_t s, bool private_gbuffer = false);
// the prepared block of mr_render_forward_l1_private (corner_rec.h: fold_private_bytes)
size_t shade_backward_private_bytes(int B, int T, int W, int H);
// the G-buffer and the specular term's across-pixels norms (norms2 [B,L], L <= 4) in one pass (raster_forward.hip)
size_t rasterize_specular_norms_ws(int B, int V, int T, int W, int H);
int launch_rasterize_specular_norms(const float *clip, const int32_t *tris, const float *normals, const float *positions,
                                    const float *light_pos, const float *camera, int B, int V, int T, int W, int H, int L,
                                    int32_t *ids, float *bary, float *z, int want_z, float *norms2, void *ws, hipStream_t s);
size_t shade_specular_forward_ws(int B, int V, int T, int W, int H);
int launch_shade_specular_forward(const int32_t *ids, const float *bary, const float *normals,
                                  const float *positions, const float *diffuse, const float *specular,
                                  const int32_t *tris, const float *light_pos, const float *light_col,
                                  const float *ambient, const float *camera, const float *shininess,
                                  int shininess_per_vertex, int B, int V, int T, int W, int H, int L,
                                  float *rgba, float *norms2, int norms2_given,
                                  void *ws, hipStream_t s);
size_t shade_specular_backward_ws(int B, int V, int T, int W, int H);
size_t shade_specular_backward_l1_ws(int B, int V, int T, int W, int H);
// signs / sign_upstream: the upstream gradient as mean|image - target|'s sign codes instead of drgba (drgba null)
int launch_shade_specular_backward(const float *drgba, const uint8_t *signs, const float *sign_upstream,
                                   const int32_t *ids, const float *bary,
                                   const float *clip, const float *normals, const float *positions,
                                   const float *diffuse, const float *specular, const int32_t *tris,
                                   const float *light_pos, const float *light_col, const float *ambient,
                                   const float *camera, const float *shininess, int shininess_per_vertex,
                                   const float *norms2, int B, int V, int T, int W, int H, int L, float *dclip,
                                   float *dnormals, float *dpositions, float *ddiffuse, float *dspecular,
                                   float *dshininess, float *light_grads, const int32_t *vertex_offsets,
                                   const int32_t *vertex_entries, const float *transforms, int gbuffer_flags,
                                   int grads_wanted, void *ws, hipStream_t s);
int launch_l1_forward(const float *a, const float *b, size_t n, float *out, uint8_t *signs, float *partials,
                      hipStream_t s);
int launch_l1_backward(const uint8_t *signs, size_t n, const float *upstream, float *da, hipStream_t s);
int launch_l1_finish(const float *partials, int n, float *out, hipStream_t s);
int launch_image_empty_regions(const float *image, int B, int H, int W, uint8_t *map, hipStream_t s);
int launch_l1_forward_regions(const float *a, const float *b, int B, int H, int W, const uint8_t *empty_a,
                              const uint8_t *empty_b, float *out, uint8_t *signs, float *partials, hipStream_t s);
int launch_export_u8(const float *in, size_t n, uint8_t *out, hipStream_t s);
int launch_vertex_normals(const float *vertices, const int32_t *tris, const int32_t *offsets,
                          const int32_t *entries, int B, int V, float *sums, float *normals, hipStream_t s);
int launch_vertex_normals_backward(const float *dnormals, const float *vertices, const float *sums,
                                   const int32_t *tris, const int32_t *offsets, const int32_t *entries,
                                   int B, int V, float *dvertices, hipStream_t s);
int launch_camera_transforms(const float *eye, const float *center, const float *up, const float *fov_y,
                             const float *near_clip, const float *far_clip, float aspect, int B, float *transforms,
                             int *degenerate, hipStream_t s);
int launch_camera_transforms_backward(const float *dtransforms, const float *eye, const float *center,
                                      const float *up, const float *fov_y, const float *near_clip,
                                      const float *far_clip, float aspect, int B, float *deye, float *dcenter,
                                      float *dup, hipStream_t s);
int launch_tone_map(const float *image, int B, size_t per_image, float gamma, int *max_bits, float *out,
                    uint8_t *out_u8, hipStream_t s);
// silhouette antialiasing (antialias.hip)
size_t antialias_backward_ws(int B, int V);
int launch_antialias_forward(const float *image, const int32_t *ids, const float *bary, const float *z,
                             const float *clip, const int32_t *tris, const int32_t *opp, int B, int V, int T, int W,
                             int H, int C, float *out, uint8_t *pair_mask, hipStream_t s);
int launch_antialias_backward(const float *dout, const float *image, const int32_t *ids, const float *bary,
                              const float *z, const float *clip, const int32_t *tris, const int32_t *opp, int B,
                              int V, int T, int W, int H, int C, float *dimage, float *dclip, void *ws,
                              hipStream_t s);
// mesh regularisers (mesh_reg.hip)
size_t mesh_regularizer_ws(int B, int V, int F);
int launch_mesh_regularizer_forward(const float *vertices, const int32_t *nbr_offsets, const int32_t *nbr,
                                    const int32_t *flaps, int B, int V, int E, int F, int terms, int use_target,
                                    float target, float *unit_dirs, float *out_terms, void *ws, hipStream_t s);
int launch_mesh_regularizer_backward(const float *dterms, const float *vertices, const float *unit_dirs,
                                     const int32_t *nbr_offsets, const int32_t *nbr, const int32_t *flaps,
                                     const int32_t *role_offsets, const int32_t *roles, int B, int V, int E, int F,
                                     int terms, int use_target, float target, float *dvertices, hipStream_t s);
// nearest neighbours between point clouds, the Chamfer distance's hot path (nearest.hip)
void nearest_plan(int B, int N, int M, int *splits, int *queries_per_lane, int *target_tile, int *workgroup);
size_t nearest_ws(int B, int N, int M);
int launch_nearest_forward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B,
                           int N, int M, float *sqdist, int32_t *idx, float *total, float weight, int accumulate,
                           void *ws, hipStream_t s);
int launch_nearest_backward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B,
                            int N, int M, const int32_t *idx_xy, const int32_t *order_xy, const int32_t *offsets_xy,
                            const int32_t *idx_yx, const int32_t *order_yx, const int32_t *offsets_yx,
                            const float *grad_points, const float *grad_images, float x_weight, float y_weight,
                            float *dx, float *dy, hipStream_t s);
// K nearest neighbours between point clouds, mr_knn_* (nearest.hip)
int knn_max_k();
void knn_plan(int B, int N, int M, int K, int *splits, int *queries_per_lane, int *list_capacity, int *target_tile,
              int *workgroup);
size_t knn_ws(int B, int N, int M, int K);
int launch_knn_forward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B, int N,
                       int M, int K, float *sqdist, int32_t *idx, void *ws, hipStream_t s);
int launch_knn_backward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B, int N,
                        int M, int K, const float *sqdist, const int32_t *idx, const int32_t *order,
                        const int32_t *offsets, const float *grad, float *dx, float *dy, hipStream_t s);
// farthest-point sampling, mr_farthest_* (farthest.hip)
int farthest_set_shape(int workgroup, int points_per_lane);
void farthest_plan(int B, int N, int K, int *route, int *workgroup, int *points_per_lane, int *slices);
size_t farthest_ws(int B, int N, int K);
int launch_farthest_forward(const float *points, const int32_t *lengths, const int32_t *start_idx, int B, int N, int K,
                            int route, int32_t *idx, float *radius, void *ws, hipStream_t s);
// (I + lam L) apply and conjugate-gradient solve over mesh_topology()'s adjacency, mr_laplacian_* (mesh_solve.hip)
bool laplacian_solve_plan(int V, int C, int route, int *chosen, int *workgroup, int *vertices_per_lane, int *slices);
size_t laplacian_solve_ws(int B, int V, int C);
int launch_laplacian_apply(const float *x, const int32_t *offsets, const int32_t *nbr, int B, int V, int C, int nnz,
                           float lam, float *y, hipStream_t s);
int launch_laplacian_solve(const float *rhs, const float *x0, const int32_t *offsets, const int32_t *nbr, int B, int V,
                           int C, int nnz, float lam, double tol, int max_iterations, int route, int first_iteration,
                           int iteration_count, int32_t *all_frozen, float *x, int32_t *iterations, float *residual,
                           void *ws, hipStream_t s);
// registration of matched point sets and ICP's per-round chain, mr_align_* (align.hip)
size_t align_ws(int B, int N);
int launch_align_solve(const float *x, const float *y, const int32_t *idx, int gather, const float *weights,
                       const float *sqdist, float max_sqdist, const int32_t *lengths, int B, int N, int M,
                       int estimate_scale, int allow_reflection, double relative_rmse_thr, float *R, float *T, float *s,
                       float *rmse, int32_t *converged, int32_t *iterations, double *prev_rmse, void *ws,
                       hipStream_t stream);
int launch_align_apply(const float *x, const int32_t *lengths, const float *R, const float *T, const float *s, int B,
                       int N, float *xt, hipStream_t stream);
int launch_align_closest_points(const float *vertices, const int32_t *triangles, const int32_t *face, const float *bary,
                                int B, int N, int V, int T, float *out, hipStream_t stream);
int launch_align_icp_init(const float *R0, const float *T0, const float *s0, int B, float *R, float *T, float *s,
                          float *rmse, int32_t *converged, int32_t *iterations, double *prev_rmse, hipStream_t stream);
// point to nearest triangle, mr_nearest_triangle_* (nearest.hip)
void nearest_triangle_plan(int B, int N, int T, int *splits, int *queries_per_lane, int *triangle_tile, int *workgroup);
size_t nearest_triangle_ws(int B, int N, int T);
int launch_nearest_triangle_forward(const float *points, const float *vertices, const int32_t *triangles,
                                    const int32_t *lengths, int B, int N, int V, int T, float *sqdist, int32_t *face,
                                    float *bary, float *total, void *ws, hipStream_t s);
int launch_nearest_triangle_backward(const float *points, const float *vertices, const int32_t *triangles,
                                     const int32_t *lengths, int B, int N, int V, int T, const int32_t *face,
                                     const float *bary, const int32_t *order, const int32_t *offsets,
                                     const float *grad_points, const float *grad_images, float *dpoints,
                                     float *dvertices, hipStream_t s);
// winding number, mr_winding_number_* (nearest.hip; the fixed-point sum: wn_fixed.h)
void winding_number_plan(int B, int N, int T, int *splits, int *queries_per_lane, int *triangle_tile, int *workgroup);
int winding_number_max_triangles();
size_t winding_number_ws(int B, int N, int T);
int launch_winding_number_forward(const float *points, const float *vertices, const int32_t *triangles,
                                  const int32_t *lengths, int B, int N, int V, int T, float *w, void *ws,
                                  hipStream_t s);

// ray casting, mr_cast_rays_* (nearest.hip): the winding number's launch shape, records and size limits
void cast_rays_plan(int B, int N, int T, int *splits, int *queries_per_lane, int *triangle_tile, int *workgroup);
size_t cast_rays_ws(int B, int N, int T);
int launch_cast_rays_forward(const float *origins, const float *directions, const float *vertices,
                             const int32_t *triangles, const int32_t *lengths, int B, int N, int V, int T, float t_min,
                             float t_max, float *t, int32_t *face, float *bary, void *ws, hipStream_t s);
int launch_cast_rays_backward(const float *directions, const float *vertices, const int32_t *triangles,
                              const int32_t *lengths, int B, int N, int V, int T, const float *t, const int32_t *face,
                              const float *bary, const int32_t *order, const int32_t *offsets, const float *grad_t,
                              float *dorigins, float *ddirections, float *dvertices, hipStream_t s);

// triangle to nearest point, mr_nearest_point_of_triangle_* (nearest.hip)
void nearest_point_of_triangle_plan(int B, int N, int T, int *splits, int *points_per_step, int *point_tile,
                                    int *workgroup);
size_t nearest_point_of_triangle_ws(int B, int N, int T);
int launch_nearest_point_of_triangle_forward(const float *points, const float *vertices, const int32_t *triangles,
                                             const int32_t *lengths, int B, int N, int V, int T, float *sqdist,
                                             int32_t *index, float *bary, float *total, int32_t *usable, void *ws,
                                             hipStream_t s);
int launch_nearest_point_of_triangle_backward(const float *points, const float *vertices, const int32_t *triangles,
                                              const int32_t *lengths, int B, int N, int V, int T,
                                              const int32_t *index, const float *bary, const int32_t *corner_order,
                                              const int32_t *corner_offsets, const int32_t *point_order,
                                              const int32_t *point_offsets, const float *grad_triangles,
                                              const float *grad_images, const int32_t *usable, float *dpoints,
                                              float *dvertices, hipStream_t s);

// spherical-harmonics shading (sh_shade.hip)
size_t sh_shade_backward_ws(int B, int W, int H);
int launch_sh_shade_forward(const float *normals, const float *diffuse, int stride, const float *alphas,
                            const float *sh, int B, int W, int H, int flip, float *rgba, hipStream_t s);
int launch_sh_shade_backward(const float *drgba, const float *normals, const float *diffuse, int stride,
                             const float *alphas, const float *sh, int B, int W, int H, int flip, float *dnormals,
                             float *ddiffuse, float *dalphas, float *dsh, void *ws, hipStream_t s);
// bilinear texture sampling (texture.hip)
size_t texture_backward_ws(int tex_batched, int Ht, int Wt, int C, int B);
int launch_texture_forward(const float *tex, int tex_batched, int Ht, int Wt, int C, const float *uv,
                           const float *mask, int B, int W, int H, int boundary, float *out, hipStream_t s);
int launch_texture_backward(const float *dout, const float *tex, int tex_batched, int Ht, int Wt, int C,
                            const float *uv, const float *mask, int B, int W, int H, int boundary, float *dtex,
                            float *duv, void *ws, hipStream_t s);
// mipmapped trilinear texture sampling and screen-space attribute derivatives (texture_mip.hip)
int texture_mip_levels(int Ht, int Wt, int max_level);
size_t texture_mip_pyramid_floats(int tex_batched, int Ht, int Wt, int C, int B, int L);
size_t texture_mip_backward_ws(int tex_batched, int Ht, int Wt, int C, int B, int L);
int launch_texture_mip_forward(const float *tex, int tex_batched, int Ht, int Wt, int C, int L, const float *uv,
                               const float *uv_da, const float *mask, int B, int W, int H, int boundary, float *pyr,
                               float *out, hipStream_t s);
int launch_texture_mip_backward(const float *dout, const float *tex, const float *pyr, int tex_batched, int Ht, int Wt,
                                int C, int L, const float *uv, const float *uv_da, const float *mask, int B, int W,
                                int H, int boundary, float *dtex, float *duv, void *ws, hipStream_t s);
int launch_attribute_derivatives(const int32_t *ids, const float *bary, const float *clip, const int32_t *tris,
                                 const float *attrs, const int32_t *attr_tris, int B, int V, int T, int Va, int W,
                                 int H, int A, float *out, hipStream_t s);
// SSIM image loss (ssim.hip)
size_t ssim_partials(int B, int H, int W, int window, int padding);
size_t ssim_plane_floats(int B, int H, int W, int C, int window, int padding);
int launch_ssim_forward(const float *a, const float *b, int B, int H, int W, int C, int window, float sigma, float c1,
                        float c2, int padding, int grads, float *mean, float *map, float *saved, float *partials,
                        hipStream_t s);
int launch_ssim_backward(const float *a, const float *b, const float *saved, const float *upstream, int B, int H, int W,
                         int C, int window, float sigma, int padding, int grads, float *da, float *db, hipStream_t s);
int soft_max_lights();
int launch_debug_soft_nearest(const float *p, const float *a, const float *b, int n, float *out, hipStream_t s);
size_t soft_ws(int B, int V, int T, int W, int H);
size_t soft_prepared_bytes(int B, int V, int T, int W, int H);
int launch_soft_forward(const float *clip, const float *positions, const float *normals,
                        const float *diffuse, const int32_t *tris, const float *lpos,
                        const float *lint, int B, int V, int T, int W, int H, int L, float sigma,
                        float gamma, float blur, float *rgba, float *aux, void *ws, hipStream_t s);
int launch_soft_backward(const float *drgba, const float *rgba, const float *aux, const float *clip,
                         const float *positions, const float *normals, const float *diffuse,
                         const int32_t *tris, const float *lpos, const float *lint, int B, int V, int T,
                         int W, int H, int L, float sigma, float gamma, float blur, float *dclip,
                         float *dpositions, float *dnormals, float *ddiffuse, float *dlpos, float *dlint,
                         const void *prepared, void *ws, hipStream_t s);

}  // namespace mr
