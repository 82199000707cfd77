// extern "C" surface of libmesh_raster_hip.so (see include/mesh_raster.h).
// Argument validation lives here; kernels and launch geometry live in the
// per-stage .hip files.  No allocation, no synchronisation, no exceptions.
#include <float.h>

#include "mr_internal.h"
#include "mesh_raster_debug.h"

namespace {

inline bool bad_dims(int B, int V, int T, int W, int H) {
  return B < 0 || V < 0 || T < 0 || W < 1 || H < 1 || W > 65535 || H > 65535;
}

inline int check_ws(const void *ws, size_t have, size_t need) {
  if (need == 0) return MR_OK;
  if (ws == nullptr || have < need) return MR_EWORKSPACE;
  if (((uintptr_t)ws & 255u) != 0) return MR_EWORKSPACE;
  return MR_OK;
}

}  // namespace

namespace mr {
extern thread_local int g_raster_region_edge;
extern thread_local int g_raster_repeat;
#ifdef MR_PROBES
extern thread_local int g_raster_probe;
#endif
thread_local KernelTimerSlot g_kernel_timers[MR_TIMER_COUNT];
extern thread_local int g_deterministic;
extern thread_local int g_shade_backward_kernel;
const char *volatile g_last_accumulate_kernel = "";
thread_local int g_lanes_rows = 0;
volatile int g_last_lanes_rows = 0;
}

extern "C" {

int mr_version(void) { return 356; /* + mr_sh_shade_forward / _backward; 355: + mr_antialias_forward / _backward; 354: + mr_rasterize_specular_norms_forward, norms2_given; 353: mr_shade_specular_backward_l1 (352: dclip optional, backward_prepared / prepared, mr_debug_soft_nearest, two's-complement sign codes) */ }

int mr_last_hip_error(void) { return mr::g_last_hip_error; }

int mr_set_deterministic(int on) {
  const int before = mr::g_deterministic;
  mr::g_deterministic = on ? 1 : 0;
  return before;
}

int mr_time_next_kernel(int which, void *start_event, void *stop_event) {
  if (which < 0 || which >= MR_TIMER_COUNT) return MR_EINVAL;
  if ((start_event == nullptr) != (stop_event == nullptr)) return MR_EINVAL;
  mr::g_kernel_timers[which].start = (hipEvent_t)start_event;
  mr::g_kernel_timers[which].stop = (hipEvent_t)stop_event;
  return MR_OK;
}

int mr_time_no_kernel(int which, void *stream) {
  if (which < 0 || which >= MR_TIMER_COUNT) return MR_EINVAL;
  { mr::KernelTimer empty_interval(which, (hipStream_t)stream); }
  return MR_OK;
}

// ---- mesh_raster_debug.h ----------------------------------------------------------------
int mr_debug_set_raster_region_edge(int edge) {
  if (edge != 0 && edge != 32 && edge != 64) return MR_EINVAL;
  mr::g_raster_region_edge = edge;
  return MR_OK;
}

int mr_debug_set_shade_backward_kernel(int which) {
  if (which < 0 || which > 2) return MR_EINVAL;
  mr::g_shade_backward_kernel = which;
  return MR_OK;
}

int mr_debug_set_raster_repeat(int n) {
  if (n < 1 || n > 64) return MR_EINVAL;
  mr::g_raster_repeat = n;
  return MR_OK;
}

const char *mr_debug_last_accumulate_kernel(void) { return mr::g_last_accumulate_kernel; }

int mr_debug_set_lanes_rows(int rows) {
  if (rows != 0 && rows != 4 && rows != 8 && rows != 16) return MR_EINVAL;
  mr::g_lanes_rows = rows;
  return MR_OK;
}

int mr_debug_last_lanes_rows(void) { return mr::g_last_lanes_rows; }

int mr_debug_set_farthest_shape(int workgroup_size, int points_per_lane) {
  return mr::farthest_set_shape(workgroup_size, points_per_lane);
}

int mr_debug_set_raster_probe(int probe) {
#ifdef MR_PROBES
  static const int kProbes[] = {0, 1, 2, 3, 8, 16, 32, 40, 48, 64};
  for (int v : kProbes) {
    if (v == probe) {
      mr::g_raster_probe = probe;
      return MR_OK;
    }
  }
  return MR_EINVAL;
#else
  return probe == 0 ? MR_OK : MR_EINVAL;  // production build: no probe code in the kernel
#endif
}

int mr_debug_soft_nearest(const float *points, const float *seg_a, const float *seg_b, int n, float *out, void *stream) {
  if (n < 0 || (n > 0 && (!points || !seg_a || !seg_b || !out))) return MR_EINVAL;
  return mr::launch_debug_soft_nearest(points, seg_a, seg_b, n, out, (hipStream_t)stream);
}

size_t mr_rasterize_forward_workspace_bytes(int B, int V, int T, int W, int H) {
  if (bad_dims(B, V, T, W, H)) return 0;
  return mr::raster_forward_ws(B, V, T, W, H);
}

int mr_rasterize_forward(const float *clip, const int32_t *triangles, int B, int V, int T, int W,
                         int H, int32_t *ids, float *bary, float *z, void *workspace,
                         size_t workspace_bytes, void *stream) {
  if (bad_dims(B, V, T, W, H)) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!ids || !bary || !z) return MR_EINVAL;
  if ((V > 0 && !clip) || (T > 0 && !triangles)) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::raster_forward_ws(B, V, T, W, H));
  if (rc != MR_OK) return rc;
  return mr::launch_raster_forward(clip, triangles, B, V, T, W, H, ids, bary, z, workspace,
                                   (hipStream_t)stream);
}

size_t mr_rasterize_backward_workspace_bytes(int B, int V, int T, int W, int H) {
  if (bad_dims(B, V, T, W, H)) return 0;
  return mr::raster_backward_ws(B, V, T, W, H);
}

int mr_rasterize_backward(const float *dbary, const float *clip, const int32_t *triangles,
                          const int32_t *ids, const float *bary, int B, int V, int T, int W,
                          int H, float *dclip, void *workspace, size_t workspace_bytes,
                          void *stream) {
  if (bad_dims(B, V, T, W, H)) return MR_EINVAL;
  if (B == 0 || V == 0) return MR_OK;
  if (!dbary || !clip || !ids || !bary || !dclip || (T > 0 && !triangles)) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::raster_backward_ws(B, V, T, W, H));
  if (rc != MR_OK) return rc;
  return mr::launch_raster_backward(dbary, clip, triangles, ids, bary, B, V, T, W, H, dclip,
                                    workspace, (hipStream_t)stream);
}

int mr_interpolate_forward(const int32_t *ids, const float *bary, const float *attrs,
                           const int32_t *triangles, const float *background, int B, int V,
                           int T, int W, int H, int A, float *out, void *stream) {
  // the reference gathers triangle 0's corners for empty pixels, so T = 0 is an error there too
  if (bad_dims(B, V, T, W, H) || A < 0 || T < 1 || V < 1) return MR_EINVAL;
  if (B == 0 || A == 0) return MR_OK;
  if (!ids || !bary || !attrs || !triangles || !background || !out) return MR_EINVAL;
  return mr::launch_interp_forward(ids, bary, attrs, triangles, background, B, V, T, W, H, A, out,
                                   (hipStream_t)stream);
}

size_t mr_interpolate_backward_workspace_bytes(int B, int V, int T, int W, int H, int A) {
  if (bad_dims(B, V, T, W, H) || A < 0) return 0;
  return mr::interp_backward_ws(B, V, T, W, H, A);
}

int mr_interpolate_backward(const float *dout, const int32_t *ids, const float *bary,
                            const float *attrs, const int32_t *triangles,
                            const float *background, int B, int V, int T, int W, int H, int A,
                            float *dattrs, float *dbary, void *workspace,
                            size_t workspace_bytes, void *stream) {
  if (bad_dims(B, V, T, W, H) || A < 0 || T < 1 || V < 1) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!dout || !ids || !bary || !attrs || !triangles || !background || !dattrs || !dbary)
    return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::interp_backward_ws(B, V, T, W, H, A));
  if (rc != MR_OK) return rc;
  return mr::launch_interp_backward(dout, ids, bary, attrs, triangles, background, B, V, T, W, H,
                                    A, dattrs, dbary, workspace, (hipStream_t)stream);
}

int mr_interpolate_raster_max_attributes(void) { return mr::interp_raster_max_attrs(); }

size_t mr_interpolate_raster_backward_workspace_bytes(int B, int V, int T, int W, int H, int A) {
  if (bad_dims(B, V, T, W, H) || A < 0 || A > mr::interp_raster_max_attrs()) return 0;
  return mr::interp_raster_backward_ws(B, V, T, W, H, A);
}

size_t mr_interpolate_records_bytes(int B, int T, int A) {
  if (B < 0 || T < 0 || A < 1 || A > mr::interp_raster_max_attrs()) return 0;
  return mr::interp_records_bytes(B, T, A);
}

int mr_interpolate_forward_records(const int32_t *ids, const float *bary, const float *attrs,
                                   const int32_t *triangles, const float *background, int B, int V,
                                   int T, int W, int H, int A, float *out, void *records,
                                   size_t records_bytes, void *stream) {
  if (bad_dims(B, V, T, W, H) || A < 1 || A > mr::interp_raster_max_attrs() || T < 1 || V < 1)
    return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!ids || !bary || !attrs || !triangles || !background || !out) return MR_EINVAL;
  const int rc = check_ws(records, records_bytes, mr::interp_records_bytes(B, T, A));
  if (rc != MR_OK) return rc;
  return mr::launch_interp_forward_records(ids, bary, attrs, triangles, background, B, V, T, W, H, A, out,
                                           records, (hipStream_t)stream);
}

int mr_rasterize_interpolate_forward(const float *clip, const float *attrs, const int32_t *triangles,
                                     const float *background, int B, int V, int T, int W, int H, int A,
                                     int32_t *ids, float *bary, float *z, float *out, void *records,
                                     size_t records_bytes, void *workspace, size_t workspace_bytes, void *stream) {
  if (bad_dims(B, V, T, W, H) || A < 1 || A > mr::interp_raster_max_attrs() || T < 1 || V < 1) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!clip || !attrs || !triangles || !background || !ids || !bary || !z || !out || ((uintptr_t)clip & 15u) ||
      ((uintptr_t)records & 255u))
    return MR_EINVAL;
  int rc = check_ws(records, records_bytes, mr::interp_records_bytes(B, T, A));
  if (rc != MR_OK) return rc;
  rc = check_ws(workspace, workspace_bytes, mr::raster_forward_ws(B, V, T, W, H));
  if (rc != MR_OK) return rc;
  return mr::launch_rasterize_interpolate_forward(clip, attrs, triangles, background, B, V, T, W, H, A, ids, bary, z, out,
                                                  records, workspace, (hipStream_t)stream);
}

int mr_interpolate_raster_backward(const float *dout, const int32_t *ids, const float *bary,
                                   const float *clip, const float *attributes,
                                   const int32_t *triangles, const float *background,
                                   const int32_t *vertex_offsets, const int32_t *vertex_entries,
                                   const void *corner_records, int B, int V, int T, int W, int H, int A,
                                   float *dattributes, float *dclip, int gbuffer_flags, void *workspace,
                                   size_t workspace_bytes, void *stream) {
  if (bad_dims(B, V, T, W, H) || A < 0 || A > mr::interp_raster_max_attrs() || (gbuffer_flags & ~MR_GBUFFER_NORMALISED))
    return MR_EINVAL;
  if (B == 0 || V == 0) return MR_OK;
  if (!dclip || (A > 0 && !dattributes)) return MR_EINVAL;
  if (((uintptr_t)dclip & 15u) != 0) return MR_EINVAL;
  if (T > 0 && A > 0 && (size_t)W * H > 0) {
    if (!dout || !ids || !bary || !clip || !attributes || !triangles || !background || !vertex_offsets ||
        !vertex_entries)
      return MR_EINVAL;
    const int rc = check_ws(workspace, workspace_bytes, mr::interp_raster_backward_ws(B, V, T, W, H, A));
    if (rc != MR_OK) return rc;
  }
  if (((uintptr_t)corner_records & 15u) != 0) return MR_EINVAL;
  return mr::launch_interp_raster_backward(dout, ids, bary, clip, attributes, triangles, background,
                                           vertex_offsets, vertex_entries, corner_records, B, V, T, W, H, A,
                                           dattributes, dclip, gbuffer_flags, workspace, (hipStream_t)stream);
}

int mr_shade_max_lights(void) { return mr::shade_max_lights(); }
int mr_shade_fast_lights(void) { return mr::shade_light_gradient_max_lights(); }

int mr_shade_forward(const int32_t *ids, const float *bary, const float *normals,
                     const float *positions, const float *diffuse, const int32_t *triangles,
                     const float *light_positions, const float *light_intensities,
                     const float *ambient, int B, int V, int T, int W, int H, int L, float *rgba,
                     void *workspace, size_t workspace_bytes, void *stream) {
  if (bad_dims(B, V, T, W, H) || T < 1 || V < 1 || L < 1 || L > mr::shade_max_lights())
    return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!ids || !bary || !normals || !positions || !diffuse || !triangles || !light_positions ||
      !light_intensities || !rgba)
    return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::shade_forward_ws(B, V, T, W, H));
  if (rc != MR_OK) return rc;
  return mr::launch_shade_forward(ids, bary, normals, positions, diffuse, triangles, light_positions,
                                  light_intensities, ambient, B, V, T, W, H, L, rgba, workspace,
                                  (hipStream_t)stream);
}

int mr_vertex_transform(const float *vertices, const float *transforms, int B, int V, float *clip,
                        void *stream) {
  if (B < 0 || V < 0) return MR_EINVAL;
  if ((size_t)B * V == 0) return MR_OK;
  if (!vertices || !transforms || !clip || ((uintptr_t)clip & 15u) || ((uintptr_t)transforms & 15u))
    return MR_EINVAL;
  return mr::launch_vertex_transform(vertices, transforms, B, V, clip, (hipStream_t)stream);
}

int mr_render_forward(const float *vertices, const float *transforms, const float *normals,
                      const float *diffuse, const int32_t *triangles, const float *light_positions,
                      const float *light_intensities, const float *ambient, int B, int V, int T, int W,
                      int H, int L, float *clip, int32_t *ids, float *bary, float *z, int want_z,
                      float *rgba, uint8_t *rgba_u8, void *corner_records, void *backward_prepared,
                      uint8_t *empty_regions, void *workspace, size_t workspace_bytes, void *stream) {
  if (bad_dims(B, V, T, W, H) || T < 1 || V < 1 || L < 1 || L > mr::shade_max_lights())
    return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!vertices || !transforms || !normals || !diffuse || !triangles || !light_positions ||
      !light_intensities || !clip || !ids || !bary || !z || !rgba || !corner_records ||
      ((uintptr_t)corner_records & 127u) || ((uintptr_t)clip & 15u) || ((uintptr_t)transforms & 15u) ||
      ((uintptr_t)rgba_u8 & 3u) || ((uintptr_t)backward_prepared & 255u))
    return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::raster_forward_ws(B, V, T, W, H));
  if (rc != MR_OK) return rc;
  return mr::launch_render_forward(vertices, transforms, normals, diffuse, triangles, light_positions,
                                   light_intensities, ambient, B, V, T, W, H, L, clip, ids, bary, z,
                                   want_z, rgba, rgba_u8, corner_records, backward_prepared, empty_regions, workspace,
                                   (hipStream_t)stream);
}

size_t mr_render_forward_l1_partials(int B, int W, int H) {
  if (B < 0 || W < 1 || H < 1 || W > 65535 || H > 65535) return 0;
  return mr::render_forward_l1_partials(B, W, H);
}

int mr_render_forward_l1(const float *vertices, const float *transforms, const float *normals,
                         const float *diffuse, const int32_t *triangles, const float *light_positions,
                         const float *light_intensities, const float *ambient, int B, int V, int T, int W,
                         int H, int L, float *clip, int32_t *ids, float *bary, float *z, int want_z,
                         float *rgba, uint8_t *rgba_u8, void *corner_records, void *backward_prepared,
                         uint8_t *empty_regions, void *workspace, size_t workspace_bytes, void *stream,
                         const float *target, const uint8_t *target_empty, float *loss, uint8_t *signs, float *partials) {
  if (bad_dims(B, V, T, W, H) || T < 1 || V < 1 || L < 1 || L > mr::shade_max_lights())
    return MR_EINVAL;
  if (!loss) return MR_EINVAL;
  if (B == 0) return mr::zero_async(loss, sizeof(float), (hipStream_t)stream) == hipSuccess ? MR_OK : mr::check_launch();
  if (!vertices || !transforms || !normals || !diffuse || !triangles || !light_positions ||
      !light_intensities || !clip || !ids || !bary || !z || !rgba || !corner_records ||
      ((uintptr_t)corner_records & 127u) || ((uintptr_t)clip & 15u) || ((uintptr_t)transforms & 15u) ||
      ((uintptr_t)rgba_u8 & 3u) || ((uintptr_t)backward_prepared & 255u) ||
      !target || ((uintptr_t)target & 15u) || !signs || !partials)
    return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::raster_forward_ws(B, V, T, W, H));
  if (rc != MR_OK) return rc;
  return mr::launch_render_forward_l1(vertices, transforms, normals, diffuse, triangles, light_positions,
                                      light_intensities, ambient, B, V, T, W, H, L, clip, ids, bary, z,
                                      want_z, rgba, rgba_u8, corner_records, backward_prepared, empty_regions, workspace,
                                      target, target_empty, loss, signs, partials, (hipStream_t)stream);
}

size_t mr_render_forward_l1_private_bytes(int B, int T, int W, int H) {
  if (B < 0 || T < 0 || W < 1 || H < 1 || W > 65535 || H > 65535) return 0;
  return mr::shade_backward_private_bytes(B, T, W, H);
}

int mr_render_forward_l1_private(const float *vertices, const float *transforms, const float *normals,
                                 const float *diffuse, const int32_t *triangles, const float *light_positions,
                                 const float *light_intensities, const float *ambient, int B, int V, int T, int W,
                                 int H, int L, float *clip, int32_t *ids, float *z, float *rgba, uint8_t *rgba_u8,
                                 void *corner_records, void *backward_private, uint8_t *empty_regions, void *workspace,
                                 size_t workspace_bytes, void *stream, const float *target, const uint8_t *target_empty,
                                 float *loss, uint8_t *signs, float *partials) {
  if (bad_dims(B, V, T, W, H) || T < 1 || V < 1 || L < 1 || L > mr::shade_max_lights())
    return MR_EINVAL;
  if (!loss) return MR_EINVAL;
  if (B == 0) return mr::zero_async(loss, sizeof(float), (hipStream_t)stream) == hipSuccess ? MR_OK : mr::check_launch();
  if (!vertices || !transforms || !normals || !diffuse || !triangles || !light_positions ||
      !light_intensities || !clip || !ids || !z || !rgba || !corner_records || !backward_private ||
      ((uintptr_t)corner_records & 127u) || ((uintptr_t)clip & 15u) || ((uintptr_t)transforms & 15u) ||
      ((uintptr_t)rgba_u8 & 3u) || ((uintptr_t)backward_private & 255u) ||
      !target || ((uintptr_t)target & 15u) || !signs || !partials)
    return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::raster_forward_ws(B, V, T, W, H));
  if (rc != MR_OK) return rc;
  return mr::launch_render_forward_l1(vertices, transforms, normals, diffuse, triangles, light_positions,
                                      light_intensities, ambient, B, V, T, W, H, L, clip, ids, nullptr, z,
                                      /*want_z=*/0, rgba, rgba_u8, corner_records, backward_private, empty_regions, workspace,
                                      target, target_empty, loss, signs, partials, (hipStream_t)stream, true);
}

size_t mr_shade_forward_workspace_bytes(int B, int V, int T, int W, int H) {
  if (bad_dims(B, V, T, W, H)) return 0;
  return mr::shade_forward_ws(B, V, T, W, H);
}

size_t mr_shade_backward_prepared_bytes(int B, int T) {
  if (B < 0 || T < 0) return 0;
  return mr::shade_backward_prepared_bytes(B, T);
}

size_t mr_shade_backward_workspace_bytes(int B, int V, int T, int W, int H) {
  if (bad_dims(B, V, T, W, H)) return 0;
  return mr::shade_backward_ws(B, V, T, W, H);
}

int mr_shade_backward(const float *drgba, const int32_t *ids, const float *bary, const float *clip,
                      const float *normals, const float *positions, const float *diffuse,
                      const int32_t *triangles, const float *light_positions,
                      const float *light_intensities, const float *ambient, int B, int V, int T,
                      int W, int H, int L, float *dclip, float *dnormals, float *dpositions,
                      float *ddiffuse, float *light_grads, const void *corner_records,
                      const int32_t *vertex_offsets, const int32_t *vertex_entries,
                      const float *transforms, int gbuffer_flags, void *prepared, const uint8_t *empty_regions,
                      void *workspace, size_t workspace_bytes, void *stream) {
  if (bad_dims(B, V, T, W, H) || T < 1 || V < 1 || L < 1 || L > mr::shade_max_lights() ||
      (gbuffer_flags & ~MR_GBUFFER_NORMALISED))
    return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!drgba || !ids || !bary || !clip || !normals || !positions || !diffuse || !triangles ||
      !light_positions || !light_intensities || (!dclip && !transforms) || !dpositions)
    return MR_EINVAL;
  if ((!dnormals || !ddiffuse) && !vertex_offsets) return MR_EINVAL;  /* only the per-vertex gather can leave outputs out */
  if (((uintptr_t)corner_records & 127u) != 0) return MR_EINVAL;
  if ((vertex_offsets == nullptr) != (vertex_entries == nullptr)) return MR_EINVAL;
  if (vertex_offsets && ((uintptr_t)dclip & 15u) != 0) return MR_EINVAL;
  if (transforms && (!vertex_offsets || ((uintptr_t)transforms & 3u) != 0)) return MR_EINVAL;
  if (((uintptr_t)prepared & 255u) != 0) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::shade_backward_ws(B, V, T, W, H));
  if (rc != MR_OK) return rc;
  return mr::launch_shade_backward(drgba, nullptr, nullptr, ids, bary, clip, normals, positions, diffuse,
                                   triangles, light_positions, light_intensities, ambient, B, V, T, W, H, L,
                                   dclip, dnormals, dpositions, ddiffuse, light_grads, corner_records,
                                   vertex_offsets, vertex_entries, transforms, gbuffer_flags, prepared, empty_regions, workspace,
                                   (hipStream_t)stream);
}

size_t mr_shade_backward_l1_workspace_bytes(int B, int V, int T, int W, int H) {
  if (bad_dims(B, V, T, W, H)) return 0;
  return mr::shade_backward_ws(B, V, T, W, H) + 256;
}

int mr_shade_backward_l1(const uint8_t *signs, const float *upstream, const int32_t *ids,
                         const float *bary, const float *clip, const float *normals,
                         const float *positions, const float *diffuse, const int32_t *triangles,
                         const float *light_positions, const float *light_intensities,
                         const float *ambient, int B, int V, int T, int W, int H, int L, float *dclip,
                         float *dnormals, float *dpositions, float *ddiffuse, float *light_grads,
                         const void *corner_records, const int32_t *vertex_offsets,
                         const int32_t *vertex_entries, const float *transforms, int gbuffer_flags,
                         void *prepared, const uint8_t *empty_regions, void *workspace, size_t workspace_bytes,
                         void *stream) {
  if (bad_dims(B, V, T, W, H) || T < 1 || V < 1 || L < 1 || L > mr::shade_max_lights() ||
      (gbuffer_flags & ~(MR_GBUFFER_NORMALISED | MR_GBUFFER_PRIVATE)))
    return MR_EINVAL;
  const bool private_gbuffer = (gbuffer_flags & MR_GBUFFER_PRIVATE) != 0;   /* no barycentric plane: `bary` is not read */
  if (private_gbuffer && (!(gbuffer_flags & MR_GBUFFER_NORMALISED) || !prepared)) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!signs || !upstream || !ids || (!bary && !private_gbuffer) || !clip || !normals || !positions || !diffuse || !triangles ||
      !light_positions || !light_intensities || (!dclip && !transforms) || !dpositions)
    return MR_EINVAL;
  if ((!dnormals || !ddiffuse) && !vertex_offsets) return MR_EINVAL;  /* only the per-vertex gather can leave outputs out */
  if (((uintptr_t)corner_records & 127u) != 0) return MR_EINVAL;
  if ((vertex_offsets == nullptr) != (vertex_entries == nullptr)) return MR_EINVAL;
  if (vertex_offsets && ((uintptr_t)dclip & 15u) != 0) return MR_EINVAL;
  if (transforms && (!vertex_offsets || ((uintptr_t)transforms & 3u) != 0)) return MR_EINVAL;
  if (((uintptr_t)prepared & 255u) != 0) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::shade_backward_ws(B, V, T, W, H) + 256);
  if (rc != MR_OK) return rc;
  return mr::launch_shade_backward(nullptr, signs, upstream, ids, bary, clip, normals, positions, diffuse,
                                   triangles, light_positions, light_intensities, ambient, B, V, T, W, H, L,
                                   dclip, dnormals, dpositions, ddiffuse, light_grads, corner_records,
                                   vertex_offsets, vertex_entries, transforms, gbuffer_flags, prepared, empty_regions, workspace,
                                   (hipStream_t)stream);
}

size_t mr_shade_specular_forward_workspace_bytes(int B, int V, int T, int W, int H) {
  if (bad_dims(B, V, T, W, H)) return 0;
  return mr::shade_specular_forward_ws(B, V, T, W, H);
}

int mr_shade_specular_forward(const int32_t *ids, const float *bary, const float *normals,
                              const float *positions, const float *diffuse, const float *specular,
                              const int32_t *triangles, const float *light_positions,
                              const float *light_intensities, const float *ambient,
                              const float *camera_position, const float *shininess,
                              int shininess_per_vertex, int B, int V, int T, int W, int H, int L,
                              float *rgba, float *norms2, int norms2_given, void *workspace, size_t workspace_bytes,
                              void *stream) {
  if (bad_dims(B, V, T, W, H) || T < 1 || V < 1 || L < 1 || L > mr::shade_light_gradient_max_lights())
    return MR_EINVAL;
  if (norms2_given != 0 && norms2_given != 1) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!ids || !bary || !normals || !positions || !diffuse || !specular || !triangles ||
      !light_positions || !light_intensities || !camera_position || !shininess || !rgba || !norms2)
    return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::shade_specular_forward_ws(B, V, T, W, H));
  if (rc != MR_OK) return rc;
  return mr::launch_shade_specular_forward(ids, bary, normals, positions, diffuse, specular, triangles,
                                           light_positions, light_intensities, ambient,
                                           camera_position, shininess, shininess_per_vertex, B, V, T, W,
                                           H, L, rgba, norms2, norms2_given,
                                           workspace, (hipStream_t)stream);
}

size_t mr_rasterize_specular_norms_workspace_bytes(int B, int V, int T, int W, int H) {
  if (bad_dims(B, V, T, W, H)) return 0;
  return mr::rasterize_specular_norms_ws(B, V, T, W, H);
}

int mr_rasterize_specular_norms_forward(const float *clip, const int32_t *triangles, const float *normals,
                                        const float *positions, const float *light_positions,
                                        const float *camera_position, int B, int V, int T, int W, int H, int L,
                                        int32_t *ids, float *bary, float *z, int want_z, float *norms2,
                                        void *workspace, size_t workspace_bytes, void *stream) {
  if (bad_dims(B, V, T, W, H) || T < 1 || V < 1 || L < 1 || L > mr::shade_light_gradient_max_lights())
    return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!clip || !triangles || !normals || !positions || !light_positions || !camera_position || !ids || !bary || !z ||
      !norms2)
    return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::rasterize_specular_norms_ws(B, V, T, W, H));
  if (rc != MR_OK) return rc;
  return mr::launch_rasterize_specular_norms(clip, triangles, normals, positions, light_positions, camera_position, B, V, T,
                                             W, H, L, ids, bary, z, want_z != 0, norms2, workspace, (hipStream_t)stream);
}

size_t mr_shade_specular_backward_workspace_bytes(int B, int V, int T, int W, int H) {
  if (bad_dims(B, V, T, W, H)) return 0;
  return mr::shade_specular_backward_ws(B, V, T, W, H);
}

int mr_shade_specular_backward(const float *drgba, const int32_t *ids, const float *bary,
                               const float *clip, const float *normals, const float *positions,
                               const float *diffuse, const float *specular,
                               const int32_t *triangles, const float *light_positions,
                               const float *light_intensities, const float *ambient,
                               const float *camera_position, const float *shininess,
                               int shininess_per_vertex, const float *norms2, int B, int V, int T,
                               int W, int H, int L, float *dclip, float *dnormals, float *dpositions,
                               float *ddiffuse, float *dspecular, float *dshininess,
                               float *light_grads, const int32_t *vertex_offsets,
                               const int32_t *vertex_entries, const float *transforms, int gbuffer_flags,
                               int grads_wanted, void *workspace, size_t workspace_bytes, void *stream) {
  if (bad_dims(B, V, T, W, H) || T < 1 || V < 1 || L < 1 || L > mr::shade_light_gradient_max_lights())
    return MR_EINVAL;
  if ((gbuffer_flags & ~MR_GBUFFER_NORMALISED) != 0 || (grads_wanted & ~MR_GRAD_ALL) != 0) return MR_EINVAL;
  if ((vertex_offsets == nullptr) != (vertex_entries == nullptr)) return MR_EINVAL;
  if (vertex_offsets && ((uintptr_t)dclip & 15u) != 0) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!drgba || !ids || !bary || !clip || !normals || !positions || !diffuse || !specular ||
      !triangles || !light_positions || !light_intensities || !camera_position || !shininess ||
      !norms2 || !dclip || !dnormals || !dpositions || !ddiffuse || !dspecular || !light_grads ||
      (shininess_per_vertex && !dshininess))
    return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::shade_specular_backward_ws(B, V, T, W, H));
  if (rc != MR_OK) return rc;
  return mr::launch_shade_specular_backward(drgba, nullptr, nullptr, ids, bary, clip, normals, positions, diffuse,
                                            specular, triangles, light_positions, light_intensities,
                                            ambient, camera_position, shininess, shininess_per_vertex,
                                            norms2, B, V, T, W, H, L, dclip, dnormals, dpositions,
                                            ddiffuse, dspecular, dshininess, light_grads, vertex_offsets,
                                            vertex_entries, transforms, gbuffer_flags, grads_wanted, workspace,
                                            (hipStream_t)stream);
}

size_t mr_shade_specular_backward_l1_workspace_bytes(int B, int V, int T, int W, int H) {
  if (bad_dims(B, V, T, W, H)) return 0;
  return mr::shade_specular_backward_l1_ws(B, V, T, W, H);
}

int mr_shade_specular_backward_l1(const uint8_t *signs, const float *upstream, const int32_t *ids,
                                  const float *bary,
                               const float *clip, const float *normals, const float *positions,
                               const float *diffuse, const float *specular,
                               const int32_t *triangles, const float *light_positions,
                               const float *light_intensities, const float *ambient,
                               const float *camera_position, const float *shininess,
                               int shininess_per_vertex, const float *norms2, int B, int V, int T,
                               int W, int H, int L, float *dclip, float *dnormals, float *dpositions,
                               float *ddiffuse, float *dspecular, float *dshininess,
                               float *light_grads, const int32_t *vertex_offsets,
                               const int32_t *vertex_entries, const float *transforms, int gbuffer_flags,
                               int grads_wanted, void *workspace, size_t workspace_bytes, void *stream) {
  if (bad_dims(B, V, T, W, H) || T < 1 || V < 1 || L < 1 || L > mr::shade_light_gradient_max_lights())
    return MR_EINVAL;
  if ((gbuffer_flags & ~MR_GBUFFER_NORMALISED) != 0 || (grads_wanted & ~MR_GRAD_ALL) != 0) return MR_EINVAL;
  if ((vertex_offsets == nullptr) != (vertex_entries == nullptr)) return MR_EINVAL;
  if (vertex_offsets && ((uintptr_t)dclip & 15u) != 0) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!signs || !upstream || !ids || !bary || !clip || !normals || !positions || !diffuse || !specular ||
      !triangles || !light_positions || !light_intensities || !camera_position || !shininess ||
      !norms2 || !dclip || !dnormals || !dpositions || !ddiffuse || !dspecular || !light_grads ||
      (shininess_per_vertex && !dshininess))
    return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::shade_specular_backward_l1_ws(B, V, T, W, H));
  if (rc != MR_OK) return rc;
  return mr::launch_shade_specular_backward(nullptr, signs, upstream, ids, bary, clip, normals, positions, diffuse,
                                            specular, triangles, light_positions, light_intensities,
                                            ambient, camera_position, shininess, shininess_per_vertex,
                                            norms2, B, V, T, W, H, L, dclip, dnormals, dpositions,
                                            ddiffuse, dspecular, dshininess, light_grads, vertex_offsets,
                                            vertex_entries, transforms, gbuffer_flags, grads_wanted, workspace,
                                            (hipStream_t)stream);
}

int mr_soft_max_lights(void) { return mr::soft_max_lights(); }

size_t mr_soft_workspace_bytes(int B, int V, int T, int W, int H) {
  if (bad_dims(B, V, T, W, H)) return 0;
  return mr::soft_ws(B, V, T, W, H);
}

size_t mr_soft_prepared_bytes(int B, int V, int T, int W, int H) {
  if (bad_dims(B, V, T, W, H)) return 0;
  return mr::soft_prepared_bytes(B, V, T, W, H);
}

int mr_soft_forward(const float *clip, const float *positions, const float *normals,
                    const float *diffuse, const int32_t *triangles, const float *light_positions,
                    const float *light_intensities, int B, int V, int T, int W, int H, int L,
                    float sigma, float gamma, float blur, float *rgba, float *aux, void *workspace,
                    size_t workspace_bytes, void *stream) {
  if (bad_dims(B, V, T, W, H) || L < 1 || L > mr::soft_max_lights() || !(sigma > 0.f) || !(gamma > 0.f))
    return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!rgba || !aux || !light_positions || !light_intensities) return MR_EINVAL;
  if (T > 0 && (!clip || !positions || !normals || !diffuse || !triangles)) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::soft_prepared_bytes(B, V, T, W, H));  // the head is all it uses
  if (rc != MR_OK) return rc;
  return mr::launch_soft_forward(clip, positions, normals, diffuse, triangles, light_positions,
                                 light_intensities, B, V, T, W, H, L, sigma, gamma, blur, rgba, aux,
                                 workspace, (hipStream_t)stream);
}

int mr_soft_backward(const float *drgba, const float *rgba, const float *aux, const float *clip,
                     const float *positions, const float *normals, const float *diffuse,
                     const int32_t *triangles, const float *light_positions,
                     const float *light_intensities, int B, int V, int T, int W, int H, int L,
                     float sigma, float gamma, float blur, float *dclip, float *dpositions,
                     float *dnormals, float *ddiffuse, float *dlight_positions,
                     float *dlight_intensities, const void *prepared, void *workspace, size_t workspace_bytes,
                     void *stream) {
  if (bad_dims(B, V, T, W, H) || L < 1 || L > mr::soft_max_lights() || !(sigma > 0.f) || !(gamma > 0.f))
    return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!drgba || !rgba || !aux || !light_positions || !light_intensities || !dlight_positions ||
      !dlight_intensities)
    return MR_EINVAL;
  if (V > 0 && (!clip || !positions || !normals || !diffuse || !dclip || !dpositions || !dnormals || !ddiffuse))
    return MR_EINVAL;
  if (T > 0 && !triangles) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::soft_ws(B, V, T, W, H));
  if (rc != MR_OK) return rc;
  return mr::launch_soft_backward(drgba, rgba, aux, clip, positions, normals, diffuse, triangles,
                                  light_positions, light_intensities, B, V, T, W, H, L, sigma, gamma,
                                  blur, dclip, dpositions, dnormals, ddiffuse, dlight_positions,
                                  dlight_intensities, prepared, workspace, (hipStream_t)stream);
}

int mr_l1_loss_partials(void) { return MR_L1_PARTIALS; }

int mr_l1_loss_forward(const float *a, const float *b, size_t n, float *loss, uint8_t *signs,
                       float *partials, void *stream) {
  if (!loss || (n > 0 && (!a || !b || !partials))) return MR_EINVAL;
  if ((((uintptr_t)a | (uintptr_t)b) & 15u) != 0) return MR_EINVAL;
  return mr::launch_l1_forward(a, b, n, loss, signs, partials, (hipStream_t)stream);
}

size_t mr_empty_regions_bytes(int B, int W, int H) {
  if (B < 0 || W < 0 || H < 0) return 0;
  return (size_t)B * ((H + 63) / 64) * ((W + 63) / 64);
}

int mr_image_empty_regions(const float *image, int B, int H, int W, uint8_t *map, void *stream) {
  if (B < 0 || H < 0 || W < 0 || H > 65535 || W > 65535) return MR_EINVAL;
  if ((size_t)B * H * W == 0) return MR_OK;
  if (!image || !map || ((uintptr_t)image & 15u)) return MR_EINVAL;
  return mr::launch_image_empty_regions(image, B, H, W, map, (hipStream_t)stream);
}

int mr_l1_loss_forward_regions(const float *a, const float *b, int B, int H, int W, const uint8_t *empty_a,
                               const uint8_t *empty_b, float *loss, uint8_t *signs, float *partials, void *stream) {
  if (B < 0 || H < 0 || W < 0 || H > 65535 || W > 65535 || !loss) return MR_EINVAL;
  if ((size_t)B * H * W > 0 && (!a || !b || !partials || !empty_a || !empty_b)) return MR_EINVAL;
  if ((((uintptr_t)a | (uintptr_t)b) & 15u) != 0) return MR_EINVAL;
  return mr::launch_l1_forward_regions(a, b, B, H, W, empty_a, empty_b, loss, signs, partials, (hipStream_t)stream);
}

int mr_l1_loss_backward(const uint8_t *signs, size_t n, const float *upstream, float *da, void *stream) {
  if (n > 0 && (!signs || !upstream || !da)) return MR_EINVAL;
  if (((uintptr_t)da & 15u) != 0) return MR_EINVAL;
  return mr::launch_l1_backward(signs, n, upstream, da, (hipStream_t)stream);
}

int mr_camera_transforms(const float *eye, const float *center, const float *up, const float *fov_y,
                         const float *near_clip, const float *far_clip, float aspect, int B, float *transforms,
                         int32_t *degenerate, void *stream) {
  if (B < 0 || !(aspect > 0.0f)) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!eye || !center || !up || !fov_y || !near_clip || !far_clip || !transforms || !degenerate) return MR_EINVAL;
  return mr::launch_camera_transforms(eye, center, up, fov_y, near_clip, far_clip, aspect, B, transforms,
                                      (int *)degenerate, (hipStream_t)stream);
}

int mr_camera_transforms_backward(const float *dtransforms, const float *eye, const float *center,
                                  const float *up, const float *fov_y, const float *near_clip,
                                  const float *far_clip, float aspect, int B, float *deye, float *dcenter,
                                  float *dup, void *stream) {
  if (B < 0 || !(aspect > 0.0f)) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!dtransforms || !eye || !center || !up || !fov_y || !near_clip || !far_clip || !deye || !dcenter || !dup)
    return MR_EINVAL;
  return mr::launch_camera_transforms_backward(dtransforms, eye, center, up, fov_y, near_clip, far_clip, aspect, B,
                                               deye, dcenter, dup, (hipStream_t)stream);
}

int mr_vertex_normals_forward(const float *vertices, const int32_t *triangles,
                              const int32_t *vertex_offsets, const int32_t *vertex_entries, int B, int V,
                              int T, float *sums, float *normals, void *stream) {
  if (B < 0 || V < 0 || T < 0) return MR_EINVAL;
  if (B == 0 || V == 0) return MR_OK;
  if (!vertices || !vertex_offsets || !sums || !normals || (T > 0 && (!triangles || !vertex_entries)))
    return MR_EINVAL;
  return mr::launch_vertex_normals(vertices, triangles, vertex_offsets, vertex_entries, B, V, sums, normals,
                                   (hipStream_t)stream);
}

int mr_vertex_normals_backward(const float *dnormals, const float *vertices, const float *sums,
                               const int32_t *triangles, const int32_t *vertex_offsets,
                               const int32_t *vertex_entries, int B, int V, int T, float *dvertices,
                               void *stream) {
  if (B < 0 || V < 0 || T < 0) return MR_EINVAL;
  if (B == 0 || V == 0) return MR_OK;
  if (!dnormals || !vertices || !sums || !vertex_offsets || !dvertices ||
      (T > 0 && (!triangles || !vertex_entries)))
    return MR_EINVAL;
  return mr::launch_vertex_normals_backward(dnormals, vertices, sums, triangles, vertex_offsets,
                                            vertex_entries, B, V, dvertices, (hipStream_t)stream);
}

inline bool bad_antialias_dims(int B, int V, int T, int W, int H, int C) {
  return bad_dims(B, V, T, W, H) || C < 1 || (size_t)B * V >= (size_t)INT_MAX ||
         (size_t)B * W * H * C >= ((size_t)1 << 40);
}

int mr_antialias_forward(const float *image, const int32_t *ids, const float *bary, const float *z,
                         const float *clip, const int32_t *triangles, const int32_t *opposite, int B, int V,
                         int T, int W, int H, int C, float *out, uint8_t *pair_mask, void *stream) {
  if (bad_antialias_dims(B, V, T, W, H, C)) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!image || !ids || !bary || !z || !out || (V > 0 && !clip) || (T > 0 && (!triangles || !opposite)))
    return MR_EINVAL;
  if (image == out || ((uintptr_t)clip & 15u) != 0) return MR_EINVAL;
  if (C == 4 && (((uintptr_t)image | (uintptr_t)out) & 15u) != 0) return MR_EINVAL;
  return mr::launch_antialias_forward(image, ids, bary, z, clip, triangles, opposite, B, V, T, W, H, C, out,
                                      pair_mask, (hipStream_t)stream);
}

size_t mr_antialias_backward_workspace_bytes(int B, int V, int T, int W, int H, int C) {
  if (bad_antialias_dims(B, V, T, W, H, C)) return 0;
  return mr::antialias_backward_ws(B, V);
}

int mr_antialias_backward(const float *dout, const float *image, const int32_t *ids, const float *bary,
                          const float *z, const float *clip, const int32_t *triangles, const int32_t *opposite,
                          int B, int V, int T, int W, int H, int C, float *dimage, float *dclip, void *workspace,
                          size_t workspace_bytes, void *stream) {
  if (bad_antialias_dims(B, V, T, W, H, C)) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!dout || !image || !ids || !bary || !z || !dimage || (V > 0 && (!clip || !dclip)) ||
      (T > 0 && (!triangles || !opposite)))
    return MR_EINVAL;
  if (dimage == dout || ((uintptr_t)clip & 15u) != 0) return MR_EINVAL;
  if (C == 4 && (((uintptr_t)dout | (uintptr_t)dimage) & 15u) != 0) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::antialias_backward_ws(B, V));
  if (rc != MR_OK) return rc;
  return mr::launch_antialias_backward(dout, image, ids, bary, z, clip, triangles, opposite, B, V, T, W, H, C,
                                       dimage, dclip, workspace, (hipStream_t)stream);
}

inline bool bad_sh_dims(int B, int W, int H, int pixel_stride) {
  return B < 0 || B > 65535 || W < 1 || H < 1 || (size_t)W * H > ((size_t)1 << 30) || pixel_stride < 3;
}

int mr_sh_shade_forward(const float *normals, const float *diffuse, int pixel_stride, const float *alphas,
                        const float *sh, int B, int W, int H, int flip, float *rgba, void *stream) {
  if (bad_sh_dims(B, W, H, pixel_stride)) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!normals || !diffuse || !sh || !rgba || ((uintptr_t)rgba & 15u) != 0) return MR_EINVAL;
  return mr::launch_sh_shade_forward(normals, diffuse, pixel_stride, alphas, sh, B, W, H, flip != 0, rgba,
                                     (hipStream_t)stream);
}

size_t mr_sh_shade_backward_workspace_bytes(int B, int W, int H) {
  if (bad_sh_dims(B, W, H, 3)) return 0;
  return mr::sh_shade_backward_ws(B, W, H);
}

int mr_sh_shade_backward(const float *drgba, const float *normals, const float *diffuse, int pixel_stride,
                         const float *alphas, const float *sh, int B, int W, int H, int flip, float *dnormals,
                         float *ddiffuse, float *dalphas, float *dsh, void *workspace, size_t workspace_bytes,
                         void *stream) {
  if (bad_sh_dims(B, W, H, pixel_stride)) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!drgba || !normals || !diffuse || !sh || ((uintptr_t)drgba & 15u) != 0) return MR_EINVAL;
  if (dalphas && !alphas) return MR_EINVAL;  // a derived alpha has no gradient
  if (dsh) {
    const int rc = check_ws(workspace, workspace_bytes, mr::sh_shade_backward_ws(B, W, H));
    if (rc != MR_OK) return rc;
  }
  return mr::launch_sh_shade_backward(drgba, normals, diffuse, pixel_stride, alphas, sh, B, W, H, flip != 0,
                                      dnormals, ddiffuse, dalphas, dsh, workspace, (hipStream_t)stream);
}

inline bool bad_mesh_reg_dims(int B, int V, int E, int F, int terms) {
  return B < 1 || B > 65535 || V < 1 || E < 0 || F < 0 || V > (1 << 28) || E > (1 << 28) || F > (1 << 28) ||
         terms < 0 || terms > (MR_MESH_LAPLACIAN | MR_MESH_EDGE | MR_MESH_NORMAL);
}

size_t mr_mesh_regularizer_workspace_bytes(int B, int V, int F) {
  if (bad_mesh_reg_dims(B, V, 0, F, 0)) return 0;
  return mr::mesh_regularizer_ws(B, V, F);
}

int mr_mesh_regularizer_forward(const float *vertices, const int32_t *nbr_offsets, const int32_t *nbr,
                                const int32_t *flaps, int B, int V, int E, int F, int terms, int use_target,
                                float target_length, float *unit_dirs, float *out_terms, void *workspace,
                                size_t workspace_bytes, void *stream) {
  if (bad_mesh_reg_dims(B, V, E, F, terms)) return MR_EINVAL;
  if (!vertices || !out_terms) return MR_EINVAL;
  if ((terms & (MR_MESH_LAPLACIAN | MR_MESH_EDGE)) && (!nbr_offsets || (E > 0 && !nbr))) return MR_EINVAL;
  if ((terms & MR_MESH_LAPLACIAN) && !unit_dirs) return MR_EINVAL;
  if ((terms & MR_MESH_NORMAL) && F > 0 && !flaps) return MR_EINVAL;
  if (terms != 0) {
    const int rc = check_ws(workspace, workspace_bytes, mr::mesh_regularizer_ws(B, V, F));
    if (rc != MR_OK) return rc;
  }
  return mr::launch_mesh_regularizer_forward(vertices, nbr_offsets, nbr, flaps, B, V, E, F, terms, use_target != 0,
                                             target_length, unit_dirs, out_terms, workspace, (hipStream_t)stream);
}

int mr_mesh_regularizer_backward(const float *dterms, const float *vertices, const float *unit_dirs,
                                 const int32_t *nbr_offsets, const int32_t *nbr, const int32_t *flaps,
                                 const int32_t *role_offsets, const int32_t *roles, int B, int V, int E, int F,
                                 int terms, int use_target, float target_length, float *dvertices, void *stream) {
  if (bad_mesh_reg_dims(B, V, E, F, terms)) return MR_EINVAL;
  if (!dterms || !vertices || !dvertices) return MR_EINVAL;
  if ((terms & (MR_MESH_LAPLACIAN | MR_MESH_EDGE)) && (!nbr_offsets || (E > 0 && !nbr))) return MR_EINVAL;
  if ((terms & MR_MESH_LAPLACIAN) && !unit_dirs) return MR_EINVAL;
  if ((terms & MR_MESH_NORMAL) && F > 0 && (!flaps || !role_offsets || !roles)) return MR_EINVAL;
  return mr::launch_mesh_regularizer_backward(dterms, vertices, unit_dirs, nbr_offsets, nbr, flaps, role_offsets,
                                              roles, B, V, E, F, terms, use_target != 0, target_length, dvertices,
                                              (hipStream_t)stream);
}

inline bool bad_texture_dims(int tex_batched, int Ht, int Wt, int C, int B, int W, int H) {
  return (tex_batched != 0 && tex_batched != 1) || Ht < 1 || Wt < 1 || Ht > 65536 || Wt > 65536 ||
         (size_t)Ht * Wt > ((size_t)1 << 28) || C < 1 || C > 4 || B < 0 || B > 65535 || W < 1 || H < 1 ||
         (size_t)W * H > ((size_t)1 << 30) ||
         (size_t)((W + 63) / 64) * (size_t)((H + 15) / 16) > ((size_t)1 << 22);  // the backward's 64 x 16 tiles
}

inline bool bad_boundary(int boundary) { return boundary != MR_TEXTURE_WRAP && boundary != MR_TEXTURE_CLAMP; }

inline bool misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

inline bool bad_ssim_dims(int B, int H, int W, int C, int window, int padding) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 65535 || W > 65535 || C < 1 || C > 4) return true;
  if (window < 3 || window > 11 || window % 2 == 0) return true;
  if (padding != MR_SSIM_SAME && padding != MR_SSIM_VALID) return true;
  if (padding == MR_SSIM_VALID && (H < window || W < window)) return true;
  return (size_t)B * H * W >= ((size_t)1 << 36);   // (16 x 32 tiles: their number stays far below 2^31)
}

inline bool bad_ssim_grads(int grads) { return grads < 0 || grads > (MR_SSIM_GRAD_IMAGE | MR_SSIM_GRAD_TARGET); }

size_t mr_ssim_partials(int B, int H, int W, int window, int padding) {
  if (bad_ssim_dims(B, H, W, 1, window, padding)) return 0;
  return mr::ssim_partials(B, H, W, window, padding);
}

size_t mr_ssim_saved_floats(int B, int H, int W, int C, int window, int padding, int grads) {
  if (bad_ssim_dims(B, H, W, C, window, padding) || bad_ssim_grads(grads) || grads == 0) return 0;
  return (size_t)(grads == (MR_SSIM_GRAD_IMAGE | MR_SSIM_GRAD_TARGET) ? 4 : 3) *
         mr::ssim_plane_floats(B, H, W, C, window, padding);
}

int mr_ssim_forward(const float *image, const float *target, int B, int H, int W, int C, int window, float sigma,
                    float c1, float c2, int padding, int grads, float *mean, float *map, float *saved, float *partials,
                    void *stream) {
  if (bad_ssim_dims(B, H, W, C, window, padding) || bad_ssim_grads(grads)) return MR_EINVAL;
  if (!(sigma > 0.0f) || !(sigma <= FLT_MAX) || !(c1 > 0.0f) || !(c2 > 0.0f) || !(c1 <= FLT_MAX) || !(c2 <= FLT_MAX))
    return MR_EINVAL;
  if (!image || !target || !mean || !partials || (grads != 0 && !saved)) return MR_EINVAL;
  if (C == 4 && (misaligned(image, 16) || misaligned(target, 16) || misaligned(map, 16) || misaligned(saved, 16)))
    return MR_EINVAL;
  return mr::launch_ssim_forward(image, target, B, H, W, C, window, sigma, c1, c2, padding, grads, mean, map,
                                 grads != 0 ? saved : nullptr, partials, (hipStream_t)stream);
}

int mr_ssim_backward(const float *image, const float *target, const float *saved, const float *upstream, int B, int H,
                     int W, int C, int window, float sigma, int padding, int grads, float *dimage, float *dtarget,
                     void *stream) {
  if (bad_ssim_dims(B, H, W, C, window, padding) || bad_ssim_grads(grads) || grads == 0) return MR_EINVAL;
  if (!(sigma > 0.0f) || !(sigma <= FLT_MAX)) return MR_EINVAL;
  if (!image || !target || !saved || !upstream) return MR_EINVAL;
  // a gradient can only be asked of the planes the forward saved for it
  if ((dimage && !(grads & MR_SSIM_GRAD_IMAGE)) || (dtarget && !(grads & MR_SSIM_GRAD_TARGET))) return MR_EINVAL;
  if (dimage == nullptr && dtarget == nullptr) return MR_OK;
  if (C == 4 && (misaligned(image, 16) || misaligned(target, 16) || misaligned(saved, 16) || misaligned(dimage, 16) ||
                 misaligned(dtarget, 16)))
    return MR_EINVAL;
  return mr::launch_ssim_backward(image, target, saved, upstream, B, H, W, C, window, sigma, padding, grads, dimage,
                                  dtarget, (hipStream_t)stream);
}

inline bool bad_nearest_dims(int B, int N, int M) {
  return B < 1 || B > 65535 || N < 1 || M < 1 || N > (1 << 28) || M > (1 << 28) ||
         (size_t)B * N >= ((size_t)1 << 36) || (size_t)B * M >= ((size_t)1 << 36);
}

int mr_nearest_plan(int B, int N, int M, int *splits, int *queries_per_lane, int *target_tile, int *workgroup_size) {
  if (bad_nearest_dims(B, N, M) || !splits || !queries_per_lane || !target_tile || !workgroup_size) return MR_EINVAL;
  mr::nearest_plan(B, N, M, splits, queries_per_lane, target_tile, workgroup_size);
  return MR_OK;
}

size_t mr_nearest_workspace_bytes(int B, int N, int M) {
  if (bad_nearest_dims(B, N, M)) return 0;
  return mr::nearest_ws(B, N, M);
}

int mr_nearest_forward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B, int N,
                       int M, float *sqdist, int32_t *idx, float *total, float weight, int accumulate, void *workspace,
                       size_t workspace_bytes, void *stream) {
  if (bad_nearest_dims(B, N, M)) return MR_EINVAL;
  if (!x || !y || !idx) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::nearest_ws(B, N, M));
  if (rc != MR_OK) return rc;
  return mr::launch_nearest_forward(x, y, x_lengths, y_lengths, B, N, M, sqdist, idx, total, weight, accumulate != 0,
                                    workspace, (hipStream_t)stream);
}

int mr_nearest_backward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B, int N,
                        int M, const int32_t *idx_xy, const int32_t *order_xy, const int32_t *offsets_xy,
                        const int32_t *idx_yx, const int32_t *order_yx, const int32_t *offsets_yx,
                        const float *grad_points, const float *grad_images, float x_weight, float y_weight, float *dx,
                        float *dy, void *stream) {
  if (bad_nearest_dims(B, N, M)) return MR_EINVAL;
  if (!x || !y) return MR_EINVAL;
  if (!idx_xy && !idx_yx) return MR_EINVAL;                       // no direction ran
  if ((grad_points != nullptr) == (grad_images != nullptr)) return MR_EINVAL;   // exactly one upstream
  if (grad_points && (!idx_xy || idx_yx)) return MR_EINVAL;       // a per-point upstream belongs to x -> y alone
  if ((order_xy == nullptr) != (offsets_xy == nullptr) || (order_yx == nullptr) != (offsets_yx == nullptr))
    return MR_EINVAL;
  // a gradient needs the scatter half of every direction that ran into its cloud
  if (dx && idx_yx && !order_yx) return MR_EINVAL;
  if (dy && idx_xy && !order_xy) return MR_EINVAL;
  return mr::launch_nearest_backward(x, y, x_lengths, y_lengths, B, N, M, idx_xy, order_xy, offsets_xy,
                                     idx_yx, order_yx, offsets_yx, grad_points, grad_images, x_weight, y_weight, dx, dy,
                                     (hipStream_t)stream);
}

inline bool bad_farthest_dims(int B, int N, int K) {
  return B < 1 || B > 65535 || N < 1 || N >= (1 << 28) || K < 1 || K >= (1 << 24) ||
         (size_t)B * K >= ((size_t)1 << 31);
}

int mr_farthest_plan(int B, int N, int K, int *route, int *workgroup_size, int *points_per_lane, int *slices) {
  if (bad_farthest_dims(B, N, K) || !route || !workgroup_size || !points_per_lane || !slices) return MR_EINVAL;
  mr::farthest_plan(B, N, K, route, workgroup_size, points_per_lane, slices);
  return MR_OK;
}

size_t mr_farthest_workspace_bytes(int B, int N, int K) {
  if (bad_farthest_dims(B, N, K)) return 0;
  return mr::farthest_ws(B, N, K);
}

int mr_farthest_forward(const float *points, const int32_t *lengths, const int32_t *start_idx, int B, int N, int K,
                        int route, int32_t *idx, float *radius, void *workspace, size_t workspace_bytes,
                        void *stream) {
  if (bad_farthest_dims(B, N, K) || route < 0 || route > 2) return MR_EINVAL;
  if (!points || !idx || !radius) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::farthest_ws(B, N, K));
  if (rc != MR_OK) return rc;
  return mr::launch_farthest_forward(points, lengths, start_idx, B, N, K, route, idx, radius, workspace,
                                     (hipStream_t)stream);
}

inline bool bad_laplacian_dims(int B, int V, int C, int nnz) {
  return B < 1 || B > 65535 || V < 1 || V >= (1 << 28) || C < 1 || C > 4 || nnz < 0 ||
         (size_t)B * V * C >= ((size_t)1 << 36);
}

inline bool bad_lam(float lam) { return !(lam >= 0.0f && lam < INFINITY); }

int mr_laplacian_apply(const float *x, const int32_t *nbr_offsets, const int32_t *nbr, int B, int V, int C, int nnz,
                       float lam, float *y, void *stream) {
  if (bad_laplacian_dims(B, V, C, nnz) || bad_lam(lam)) return MR_EINVAL;
  if (!x || !y || !nbr_offsets || (nnz > 0 && !nbr)) return MR_EINVAL;
  return mr::launch_laplacian_apply(x, nbr_offsets, nbr, B, V, C, nnz, lam, y, (hipStream_t)stream);
}

int mr_laplacian_solve_plan(int V, int C, int route, int *chosen_route, int *workgroup_size, int *vertices_per_lane,
                            int *slices) {
  if (bad_laplacian_dims(1, V, C, 0) || route < 0 || route > 2) return MR_EINVAL;
  if (!chosen_route || !workgroup_size || !vertices_per_lane || !slices) return MR_EINVAL;
  return mr::laplacian_solve_plan(V, C, route, chosen_route, workgroup_size, vertices_per_lane, slices) ? MR_OK
                                                                                                        : MR_EINVAL;
}

size_t mr_laplacian_solve_workspace_bytes(int B, int V, int C) {
  if (bad_laplacian_dims(B, V, C, 0)) return 0;
  return mr::laplacian_solve_ws(B, V, C);
}

int mr_laplacian_solve(const float *b, const float *x0, const int32_t *nbr_offsets, const int32_t *nbr, int B, int V,
                       int C, int nnz, float lam, double tol, int max_iterations, int route, int first_iteration,
                       int iteration_count, int32_t *all_frozen, float *x, int32_t *iterations, float *residual,
                       void *workspace, size_t workspace_bytes, void *stream) {
  if (bad_laplacian_dims(B, V, C, nnz) || bad_lam(lam) || route < 0 || route > 2) return MR_EINVAL;
  if (!(tol >= 0.0 && tol < (double)INFINITY) || max_iterations < 0 || max_iterations > 10000) return MR_EINVAL;
  if (first_iteration < 0 || first_iteration > max_iterations || iteration_count < 0) return MR_EINVAL;
  if (!b || !x || !iterations || !residual || !nbr_offsets || (nnz > 0 && !nbr)) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::laplacian_solve_ws(B, V, C));
  if (rc != MR_OK) return rc;
  return mr::launch_laplacian_solve(b, x0, nbr_offsets, nbr, B, V, C, nnz, lam, tol, max_iterations, route,
                                    first_iteration, iteration_count, all_frozen, x, iterations, residual, workspace,
                                    (hipStream_t)stream);
}

size_t mr_align_workspace_bytes(int B, int N) {
  if (bad_nearest_dims(B, N, 1)) return 0;
  return mr::align_ws(B, N);
}

int mr_align_solve(const float *x, const float *y, const int32_t *idx, int gather, const float *weights,
                   const float *sqdist, float max_sqdist, const int32_t *lengths, int B, int N, int M,
                   int estimate_scale, int allow_reflection, double relative_rmse_thr, float *R, float *T, float *s,
                   float *rmse, int32_t *converged, int32_t *iterations, double *prev_rmse, void *workspace,
                   size_t workspace_bytes, void *stream) {
  if (bad_nearest_dims(B, N, M)) return MR_EINVAL;
  if (!x || !y || !R || !T || !s) return MR_EINVAL;
  if (gather ? !idx : M != N) return MR_EINVAL;   // row by row: y has x's rows
  const bool icp = converged != nullptr;
  if ((iterations != nullptr) != icp || (prev_rmse != nullptr) != icp || (icp && !rmse)) return MR_EINVAL;
  if (misaligned(prev_rmse, 8)) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::align_ws(B, N));
  if (rc != MR_OK) return rc;
  return mr::launch_align_solve(x, y, idx, gather != 0, weights, sqdist, max_sqdist, lengths, B, N, M,
                                estimate_scale != 0, allow_reflection != 0, relative_rmse_thr, R, T, s, rmse, converged,
                                iterations, prev_rmse, workspace, (hipStream_t)stream);
}

int mr_align_apply(const float *x, const int32_t *lengths, const float *R, const float *T, const float *s, int B, int N,
                   float *xt, void *stream) {
  if (bad_nearest_dims(B, N, 1)) return MR_EINVAL;
  if (!x || !R || !T || !s || !xt) return MR_EINVAL;
  return mr::launch_align_apply(x, lengths, R, T, s, B, N, xt, (hipStream_t)stream);
}

int mr_align_closest_points(const float *vertices, const int32_t *triangles, const int32_t *face, const float *bary,
                            int B, int N, int V, int T, float *out, void *stream) {
  if (bad_nearest_dims(B, N, T) || V < 1 || V > (1 << 28) || (size_t)B * V >= ((size_t)1 << 36)) return MR_EINVAL;
  if (!vertices || !triangles || !face || !bary || !out) return MR_EINVAL;
  return mr::launch_align_closest_points(vertices, triangles, face, bary, B, N, V, T, out, (hipStream_t)stream);
}

int mr_align_icp_init(const float *R0, const float *T0, const float *s0, int B, float *R, float *T, float *s,
                      float *rmse, int32_t *converged, int32_t *iterations, double *prev_rmse, void *stream) {
  if (B < 1 || B > 65535) return MR_EINVAL;
  if (!R || !T || !s || !rmse || !converged || !iterations || !prev_rmse || misaligned(prev_rmse, 8)) return MR_EINVAL;
  if ((R0 != nullptr) != (T0 != nullptr) || (R0 != nullptr) != (s0 != nullptr)) return MR_EINVAL;
  return mr::launch_align_icp_init(R0, T0, s0, B, R, T, s, rmse, converged, iterations, prev_rmse, (hipStream_t)stream);
}

inline bool bad_knn_dims(int B, int N, int M, int K) {
  return bad_nearest_dims(B, N, M) || K < 1 || K > mr::knn_max_k() || (size_t)N * K > (size_t)INT_MAX ||
         (size_t)B * N * K >= ((size_t)1 << 36);
}

int mr_knn_plan(int B, int N, int M, int K, int *splits, int *queries_per_lane, int *list_capacity, int *target_tile,
                int *workgroup_size) {
  if (bad_knn_dims(B, N, M, K) || !splits || !queries_per_lane || !list_capacity || !target_tile || !workgroup_size)
    return MR_EINVAL;
  mr::knn_plan(B, N, M, K, splits, queries_per_lane, list_capacity, target_tile, workgroup_size);
  return MR_OK;
}

size_t mr_knn_workspace_bytes(int B, int N, int M, int K) {
  if (bad_knn_dims(B, N, M, K)) return 0;
  return mr::knn_ws(B, N, M, K);
}

int mr_knn_forward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B, int N,
                   int M, int K, float *sqdist, int32_t *idx, void *workspace, size_t workspace_bytes, void *stream) {
  if (bad_knn_dims(B, N, M, K)) return MR_EINVAL;
  if (!x || !y || !sqdist || !idx) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::knn_ws(B, N, M, K));
  if (rc != MR_OK) return rc;
  return mr::launch_knn_forward(x, y, x_lengths, y_lengths, B, N, M, K, sqdist, idx, workspace, (hipStream_t)stream);
}

int mr_knn_backward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B, int N,
                    int M, int K, const float *sqdist, const int32_t *idx, const int32_t *order, const int32_t *offsets,
                    const float *grad, float *dx, float *dy, void *stream) {
  if (bad_knn_dims(B, N, M, K)) return MR_EINVAL;
  if (!x || !y || !sqdist || !idx || !grad) return MR_EINVAL;
  if ((order == nullptr) != (offsets == nullptr)) return MR_EINVAL;
  if (dy && !order) return MR_EINVAL;   // the targets' gradient is a gather over the inverted index
  return mr::launch_knn_backward(x, y, x_lengths, y_lengths, B, N, M, K, sqdist, idx, order, offsets, grad, dx, dy,
                                 (hipStream_t)stream);
}

inline bool bad_nearest_triangle_dims(int B, int N, int V, int T) {
  return bad_nearest_dims(B, N, T) || V < 1 || V > (1 << 28) || (size_t)B * V >= ((size_t)1 << 36);
}

int mr_nearest_triangle_plan(int B, int N, int T, int *splits, int *queries_per_lane, int *triangle_tile,
                             int *workgroup_size) {
  if (bad_nearest_dims(B, N, T) || !splits || !queries_per_lane || !triangle_tile || !workgroup_size) return MR_EINVAL;
  mr::nearest_triangle_plan(B, N, T, splits, queries_per_lane, triangle_tile, workgroup_size);
  return MR_OK;
}

size_t mr_nearest_triangle_workspace_bytes(int B, int N, int T) {
  if (bad_nearest_dims(B, N, T)) return 0;
  return mr::nearest_triangle_ws(B, N, T);
}

int mr_nearest_triangle_forward(const float *points, const float *vertices, const int32_t *triangles,
                                const int32_t *lengths, int B, int N, int V, int T, float *sqdist, int32_t *face,
                                float *bary, float *total, void *workspace, size_t workspace_bytes, void *stream) {
  if (bad_nearest_triangle_dims(B, N, V, T)) return MR_EINVAL;
  if (!points || !vertices || !triangles || !face || !bary) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::nearest_triangle_ws(B, N, T));
  if (rc != MR_OK) return rc;
  if (misaligned(workspace, 16)) return MR_EINVAL;   // the records are read as 16-byte words
  return mr::launch_nearest_triangle_forward(points, vertices, triangles, lengths, B, N, V, T, sqdist, face, bary, total,
                                             workspace, (hipStream_t)stream);
}

int mr_nearest_triangle_backward(const float *points, const float *vertices, const int32_t *triangles,
                                 const int32_t *lengths, int B, int N, int V, int T, const int32_t *face,
                                 const float *bary, const int32_t *order, const int32_t *offsets,
                                 const float *grad_points, const float *grad_images, float *dpoints, float *dvertices,
                                 void *stream) {
  if (bad_nearest_triangle_dims(B, N, V, T)) return MR_EINVAL;
  if (!points || !vertices || !triangles || !face || !bary) return MR_EINVAL;
  if ((grad_points != nullptr) == (grad_images != nullptr)) return MR_EINVAL;   // exactly one upstream
  if ((order == nullptr) != (offsets == nullptr)) return MR_EINVAL;
  if (dvertices && !order) return MR_EINVAL;                      // the vertices' gradient is a gather over the index
  return mr::launch_nearest_triangle_backward(points, vertices, triangles, lengths, B, N, V, T, face, bary, order,
                                              offsets, grad_points, grad_images, dpoints, dvertices,
                                              (hipStream_t)stream);
}

// the fixed-point sum of 2^24 terms of at most half a turn each is the last that cannot leave the 64-bit range
inline bool bad_winding_number_dims(int B, int N, int T) {
  return bad_nearest_dims(B, N, T) || T > mr::winding_number_max_triangles();
}

int mr_winding_number_plan(int B, int N, int T, int *splits, int *queries_per_lane, int *triangle_tile,
                           int *workgroup_size) {
  if (bad_winding_number_dims(B, N, T) || !splits || !queries_per_lane || !triangle_tile || !workgroup_size)
    return MR_EINVAL;
  mr::winding_number_plan(B, N, T, splits, queries_per_lane, triangle_tile, workgroup_size);
  return MR_OK;
}

size_t mr_winding_number_workspace_bytes(int B, int N, int T) {
  if (bad_winding_number_dims(B, N, T)) return 0;
  return mr::winding_number_ws(B, N, T);
}

int mr_winding_number_forward(const float *points, const float *vertices, const int32_t *triangles,
                              const int32_t *lengths, int B, int N, int V, int T, float *w, void *workspace,
                              size_t workspace_bytes, void *stream) {
  if (bad_nearest_triangle_dims(B, N, V, T) || bad_winding_number_dims(B, N, T)) return MR_EINVAL;
  if (!points || !vertices || !triangles || !w) return MR_EINVAL;
  const int rc = check_ws(workspace, workspace_bytes, mr::winding_number_ws(B, N, T));
  if (rc != MR_OK) return rc;
  if (misaligned(workspace, 16)) return MR_EINVAL;   // the records are read as 16-byte words
  return mr::launch_winding_number_forward(points, vertices, triangles, lengths, B, N, V, T, w, workspace,
                                           (hipStream_t)stream);
}

// ray casting keeps the winding number's size limits
int mr_cast_rays_plan(int B, int N, int T, int *splits, int *queries_per_lane, int *triangle_tile,
                      int *workgroup_size) {
  if (bad_winding_number_dims(B, N, T) || !splits || !queries_per_lane || !triangle_tile || !workgroup_size)
    return MR_EINVAL;
  mr::cast_rays_plan(B, N, T, splits, queries_per_lane, triangle_tile, workgroup_size);
  return MR_OK;
}

size_t mr_cast_rays_workspace_bytes(int B, int N, int T) {
  if (bad_winding_number_dims(B, N, T)) return 0;
  return mr::cast_rays_ws(B, N, T);
}

int mr_cast_rays_forward(const float *origins, const float *directions, const float *vertices,
                         const int32_t *triangles, const int32_t *lengths, int B, int N, int V, int T, float t_min,
                         float t_max, float *t, int32_t *face, float *bary, void *workspace, size_t workspace_bytes,
                         void *stream) {
  if (bad_nearest_triangle_dims(B, N, V, T) || bad_winding_number_dims(B, N, T)) return MR_EINVAL;
  if (!origins || !directions || !vertices || !triangles || !t || !face || !bary) return MR_EINVAL;
  if (!(t_min >= 0.0f && t_min <= t_max)) return MR_EINVAL;   // a NaN fails
  const int rc = check_ws(workspace, workspace_bytes, mr::cast_rays_ws(B, N, T));
  if (rc != MR_OK) return rc;
  if (misaligned(workspace, 16)) return MR_EINVAL;   // the records are read as 16-byte words
  return mr::launch_cast_rays_forward(origins, directions, vertices, triangles, lengths, B, N, V, T, t_min, t_max, t,
                                      face, bary, workspace, (hipStream_t)stream);
}

int mr_cast_rays_backward(const float *directions, const float *vertices, const int32_t *triangles,
                          const int32_t *lengths, int B, int N, int V, int T, const float *t, const int32_t *face,
                          const float *bary, const int32_t *order, const int32_t *offsets, const float *grad_t,
                          float *dorigins, float *ddirections, float *dvertices, void *stream) {
  if (bad_nearest_triangle_dims(B, N, V, T) || bad_winding_number_dims(B, N, T)) return MR_EINVAL;
  if (!directions || !vertices || !triangles || !t || !face || !bary || !grad_t) return MR_EINVAL;
  if ((order == nullptr) != (offsets == nullptr)) return MR_EINVAL;
  if (dvertices && !order) return MR_EINVAL;                      // the vertices' gradient is a gather over the index
  return mr::launch_cast_rays_backward(directions, vertices, triangles, lengths, B, N, V, T, t, face, bary, order,
                                       offsets, grad_t, dorigins, ddirections, dvertices, (hipStream_t)stream);
}

int mr_nearest_point_of_triangle_plan(int B, int N, int T, int *splits, int *points_per_step, int *point_tile,
                                      int *workgroup_size) {
  if (bad_nearest_dims(B, N, T) || !splits || !points_per_step || !point_tile || !workgroup_size) return MR_EINVAL;
  mr::nearest_point_of_triangle_plan(B, N, T, splits, points_per_step, point_tile, workgroup_size);
  return MR_OK;
}

size_t mr_nearest_point_of_triangle_workspace_bytes(int B, int N, int T) {
  if (bad_nearest_dims(B, N, T)) return 0;
  return mr::nearest_point_of_triangle_ws(B, N, T);
}

int mr_nearest_point_of_triangle_forward(const float *points, const float *vertices, const int32_t *triangles,
                                         const int32_t *lengths, int B, int N, int V, int T, float *sqdist,
                                         int32_t *index, float *bary, float *total, int32_t *usable, void *workspace,
                                         size_t workspace_bytes, void *stream) {
  if (bad_nearest_triangle_dims(B, N, V, T)) return MR_EINVAL;
  if (!points || !vertices || !triangles || !index || !bary) return MR_EINVAL;
  if (total && !usable) return MR_EINVAL;   // the mean's divisor is formed on the device
  const int rc = check_ws(workspace, workspace_bytes, mr::nearest_point_of_triangle_ws(B, N, T));
  if (rc != MR_OK) return rc;
  if (misaligned(workspace, 16)) return MR_EINVAL;   // the records are read as 16-byte words
  return mr::launch_nearest_point_of_triangle_forward(points, vertices, triangles, lengths, B, N, V, T, sqdist, index,
                                                      bary, total, usable, workspace, (hipStream_t)stream);
}

int mr_nearest_point_of_triangle_backward(const float *points, const float *vertices, const int32_t *triangles,
                                          const int32_t *lengths, int B, int N, int V, int T, const int32_t *index,
                                          const float *bary, const int32_t *corner_order,
                                          const int32_t *corner_offsets, const int32_t *point_order,
                                          const int32_t *point_offsets, const float *grad_triangles,
                                          const float *grad_images, const int32_t *usable, float *dpoints,
                                          float *dvertices, void *stream) {
  if (bad_nearest_triangle_dims(B, N, V, T)) return MR_EINVAL;
  if (!points || !vertices || !triangles || !index || !bary) return MR_EINVAL;
  if ((grad_triangles != nullptr) == (grad_images != nullptr)) return MR_EINVAL;   // exactly one upstream
  if (grad_images && !usable) return MR_EINVAL;                   // the mean's upstream is divided by the count
  if ((corner_order == nullptr) != (corner_offsets == nullptr) || (point_order == nullptr) != (point_offsets == nullptr))
    return MR_EINVAL;
  if ((dvertices && !corner_order) || (dpoints && !point_order)) return MR_EINVAL;   // both are gathers over an index
  return mr::launch_nearest_point_of_triangle_backward(points, vertices, triangles, lengths, B, N, V, T, index, bary,
                                                       corner_order, corner_offsets, point_order, point_offsets,
                                                       grad_triangles, grad_images, usable, dpoints, dvertices,
                                                       (hipStream_t)stream);
}

int mr_texture_forward(const float *tex, const float *uv, const float *mask, int tex_batched, int Ht, int Wt, int C,
                       int B, int W, int H, int boundary, float *out, void *stream) {
  if (bad_texture_dims(tex_batched, Ht, Wt, C, B, W, H) || bad_boundary(boundary)) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!tex || !uv || !out || misaligned(tex, 16) || misaligned(out, 16) || misaligned(uv, 8)) return MR_EINVAL;
  return mr::launch_texture_forward(tex, tex_batched, Ht, Wt, C, uv, mask, B, W, H, boundary, out,
                                    (hipStream_t)stream);
}

size_t mr_texture_backward_workspace_bytes(int tex_batched, int Ht, int Wt, int C, int B, int W, int H) {
  if (bad_texture_dims(tex_batched, Ht, Wt, C, B, W, H)) return 0;
  return mr::texture_backward_ws(tex_batched, Ht, Wt, C, B);
}

int mr_texture_backward(const float *dout, const float *tex, const float *uv, const float *mask, int tex_batched,
                        int Ht, int Wt, int C, int B, int W, int H, int boundary, float *dtex, float *duv,
                        void *workspace, size_t workspace_bytes, void *stream) {
  if (bad_texture_dims(tex_batched, Ht, Wt, C, B, W, H) || bad_boundary(boundary)) return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!dout || !tex || !uv || misaligned(dout, 16) || misaligned(tex, 16) || misaligned(uv, 8)) return MR_EINVAL;
  if ((dtex && misaligned(dtex, 16)) || (duv && misaligned(duv, 8))) return MR_EINVAL;
  if (dtex) {
    const int rc = check_ws(workspace, workspace_bytes, mr::texture_backward_ws(tex_batched, Ht, Wt, C, B));
    if (rc != MR_OK) return rc;
  }
  return mr::launch_texture_backward(dout, tex, tex_batched, Ht, Wt, C, uv, mask, B, W, H, boundary, dtex, duv,
                                     workspace, (hipStream_t)stream);
}

int mr_texture_mip_levels(int Ht, int Wt, int max_level) {
  if (Ht < 1 || Wt < 1 || Ht > 65536 || Wt > 65536) return 0;
  return mr::texture_mip_levels(Ht, Wt, max_level);
}

size_t mr_texture_mip_pyramid_bytes(int tex_batched, int Ht, int Wt, int C, int B, int max_level) {
  if (bad_texture_dims(tex_batched, Ht, Wt, C, B, 1, 1)) return 0;
  return mr::texture_mip_pyramid_floats(tex_batched, Ht, Wt, C, B, mr::texture_mip_levels(Ht, Wt, max_level)) *
         sizeof(float);
}

int mr_texture_mip_forward(const float *tex, const float *uv, const float *uv_da, const float *mask, int tex_batched,
                           int Ht, int Wt, int C, int B, int W, int H, int boundary, int max_level, float *pyramid,
                           float *out, void *stream) {
  if (bad_texture_dims(tex_batched, Ht, Wt, C, B, W, H) || bad_boundary(boundary)) return MR_EINVAL;
  if (B == 0) return MR_OK;
  const int L = mr::texture_mip_levels(Ht, Wt, max_level);
  if (!tex || !uv || !uv_da || !out || misaligned(tex, 16) || misaligned(out, 16) || misaligned(uv, 8) ||
      misaligned(uv_da, 16))
    return MR_EINVAL;
  if (L > 1 && (!pyramid || misaligned(pyramid, 16))) return MR_EINVAL;
  return mr::launch_texture_mip_forward(tex, tex_batched, Ht, Wt, C, L, uv, uv_da, mask, B, W, H, boundary, pyramid,
                                        out, (hipStream_t)stream);
}

size_t mr_texture_mip_backward_workspace_bytes(int tex_batched, int Ht, int Wt, int C, int B, int W, int H,
                                               int max_level) {
  if (bad_texture_dims(tex_batched, Ht, Wt, C, B, W, H)) return 0;
  return mr::texture_mip_backward_ws(tex_batched, Ht, Wt, C, B, mr::texture_mip_levels(Ht, Wt, max_level));
}

int mr_texture_mip_backward(const float *dout, const float *tex, const float *pyramid, const float *uv,
                            const float *uv_da, const float *mask, int tex_batched, int Ht, int Wt, int C, int B,
                            int W, int H, int boundary, int max_level, float *dtex, float *duv, void *workspace,
                            size_t workspace_bytes, void *stream) {
  if (bad_texture_dims(tex_batched, Ht, Wt, C, B, W, H) || bad_boundary(boundary)) return MR_EINVAL;
  if (B == 0) return MR_OK;
  const int L = mr::texture_mip_levels(Ht, Wt, max_level);
  if (!dout || !tex || !uv || !uv_da || misaligned(dout, 16) || misaligned(tex, 16) || misaligned(uv, 8) ||
      misaligned(uv_da, 16))
    return MR_EINVAL;
  if (L > 1 && (!pyramid || misaligned(pyramid, 16))) return MR_EINVAL;
  if ((dtex && misaligned(dtex, 16)) || (duv && misaligned(duv, 8))) return MR_EINVAL;
  if (dtex) {
    const int rc = check_ws(workspace, workspace_bytes, mr::texture_mip_backward_ws(tex_batched, Ht, Wt, C, B, L));
    if (rc != MR_OK) return rc;
  }
  return mr::launch_texture_mip_backward(dout, tex, pyramid, tex_batched, Ht, Wt, C, L, uv, uv_da, mask, B, W, H,
                                         boundary, dtex, duv, workspace, (hipStream_t)stream);
}

int mr_attribute_derivatives(const int32_t *ids, const float *bary, const float *clip, const int32_t *triangles,
                             const float *attributes, const int32_t *attribute_triangles, int B, int V, int T,
                             int Va, int W, int H, int A, float *out, void *stream) {
  if (bad_dims(B, V, T, W, H) || A < 1 || A > 4 || T < 1 || V < 1 || Va < 1 || B > 65535 ||
      (size_t)W * H > ((size_t)1 << 30))
    return MR_EINVAL;
  if (B == 0) return MR_OK;
  if (!ids || !bary || !clip || !triangles || !attributes || !out || misaligned(clip, 16) || misaligned(out, 8))
    return MR_EINVAL;
  return mr::launch_attribute_derivatives(ids, bary, clip, triangles, attributes, attribute_triangles, B, V, T, Va, W,
                                          H, A, out, (hipStream_t)stream);
}

int mr_tone_map(const float *image, int B, size_t elements_per_image, float gamma, int32_t *max_scratch,
                float *out_f32, uint8_t *out_u8, void *stream) {
  if (B < 0) return MR_EINVAL;
  if (B == 0 || elements_per_image == 0) return MR_OK;
  if (!image || !max_scratch || ((out_f32 == nullptr) == (out_u8 == nullptr))) return MR_EINVAL;
  return mr::launch_tone_map(image, B, elements_per_image, gamma, (int *)max_scratch, out_f32, out_u8,
                             (hipStream_t)stream);
}

int mr_export_u8(const float *image, size_t n, uint8_t *out, void *stream) {
  if (n > 0 && (!image || !out)) return MR_EINVAL;
  if (((uintptr_t)image & 15u) != 0 || ((uintptr_t)out & 3u) != 0) return MR_EINVAL;
  return mr::launch_export_u8(image, n, out, (hipStream_t)stream);
}

}  // extern "C"
