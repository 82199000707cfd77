/*
 * mesh_raster.h -- C ABI of the MI355X (gfx950) differentiable mesh rasterizer.
 *
 * Drop-in boundary for the reference's one native module, the pybind11
 * extension `rasterize_triangles_cpp`
 *   (src/mesh_renderer/kernels/rasterize_triangles.cpp:421-424), whose only
 * caller is BarycentricRasterizer (src/mesh_renderer/rasterize_triangles_ext.py
 * :39-40 forward, :56-61 backward).  The interpolation / shading entry points
 * replace the eager-torch bodies of rasterize_clip_space
 * (src/mesh_renderer/rasterize.py:112-150) and phong_shader
 * (src/mesh_renderer/render.py:287-386).
 *
 * Conventions for every entry point
 *   - all data pointers are DEVICE pointers (HBM resident), contiguous, C order;
 *   - the caller owns every buffer, outputs included; nothing is allocated or
 *     freed here, so a call sequence can be captured into a hipGraph;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 *     legacy default stream) and the call returns without synchronising;
 *   - `workspace` is scratch the call may overwrite; its minimum size comes
 *     from the matching *_workspace_bytes() query, 256-byte aligned;
 *   - return value: MR_OK or a negative MR_E* code; no exceptions cross the ABI;
 *   - batched: B independent images share one `triangles` array; the
 *     reference's per-image call is B = 1.
 *
 * Numerical contract: mr_rasterize_forward reproduces the reference's ids, z
 * and barycentrics BIT FOR BIT (un-fused binary32 arithmetic in the
 * reference's evaluation order, binary64 pixel centres / bbox projection;
 * SURVEY.md Appendix A).  Gradients agree within 1e-4 abs (summation order
 * differs: LDS/atomic accumulation instead of a serial row-major loop).
 */
#ifndef MESH_RASTER_H_
#define MESH_RASTER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MR_OK 0
#define MR_EINVAL (-1)     /* null pointer, negative count, W/H out of [1, 65535] */
#define MR_EWORKSPACE (-2) /* workspace missing, too small or misaligned */
#define MR_ELAUNCH (-3)    /* a HIP launch / memset failed (see mr_last_hip_error) */

/* Library / ABI version: major*10000 + minor*100 + patch. */
int mr_version(void);
/* hipError_t of the most recent failed launch in this process, 0 if none. */
int mr_last_hip_error(void);

/* ---- rasterize_triangles_cpp.forward -------------------------------------
 * Replaces rasterize_triangles_forward (rasterize_triangles.cpp:302-419).
 *   clip      [B,V,4] f32  clip-space XYZW
 *   triangles [T,3]   i32  vertex ids (a triangle with an id outside [0,V) is
 *                          skipped; the reference would read out of bounds)
 *   ids       [B,H,W]   i32 out  winning triangle id, 0 where nothing was drawn
 *   bary      [B,H,W,3] f32 out  perspective-correct barycentrics, 0 where empty
 *   z         [B,H,W]   f32 out  NDC depth of the winner, 1.0 where empty
 * Row 0 is the BOTTOM scanline (NDC y = -1), as in the reference. */
size_t mr_rasterize_forward_workspace_bytes(int B, int V, int T, int W, int H);
int mr_rasterize_forward(const float *clip, const int32_t *triangles,
                         int B, int V, int T, int W, int H,
                         int32_t *ids, float *bary, float *z,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---- rasterize_triangles_cpp.backward ------------------------------------
 * Replaces rasterize_triangles_backward (rasterize_triangles.cpp:131-273).
 *   dbary [B,H,W,3] f32   dL/d(bary)
 *   ids, bary             the forward's outputs
 *   dclip [B,V,4] f32 out dL/d(clip); zeroed here; column 2 (z) stays 0 */
size_t mr_rasterize_backward_workspace_bytes(int B, int V, int T, int W, int H);
int mr_rasterize_backward(const float *dbary, const float *clip,
                          const int32_t *triangles, const int32_t *ids,
                          const float *bary, int B, int V, int T, int W, int H,
                          float *dclip, void *workspace, size_t workspace_bytes,
                          void *stream);

/* ---- deferred attribute interpolation -------------------------------------
 * Replaces the gather / multiply / sum / alpha / background-blend block of
 * rasterize_clip_space (src/mesh_renderer/rasterize.py:118-150).
 *   attrs      [B,V,A] f32
 *   background [A]     f32
 *   out        [B,H,W,A] f32 out (not flipped) */
int mr_interpolate_forward(const int32_t *ids, const float *bary,
                           const float *attrs, const int32_t *triangles,
                           const float *background, int B, int V, int T,
                           int W, int H, int A, float *out, void *stream);

/* Its autograd backward (index_put_(accumulate) + d/d bary).
 *   dout   [B,H,W,A] f32
 *   dattrs [B,V,A]   f32 out, zeroed here
 *   dbary  [B,H,W,3] f32 out */
size_t mr_interpolate_backward_workspace_bytes(int B, int V, int T, int W, int H, int A);
int mr_interpolate_backward(const float *dout, const int32_t *ids,
                            const float *bary, const float *attrs,
                            const int32_t *triangles, const float *background,
                            int B, int V, int T, int W, int H, int A,
                            float *dattrs, float *dbary, void *workspace,
                            size_t workspace_bytes, void *stream);

/* Backward of mr_interpolate_forward AND of the rasterizer underneath it in ONE pass over the
 * G-buffer, for 1 <= A <= mr_interpolate_raster_max_attributes() (replaces the pair
 * mr_interpolate_backward + mr_rasterize_backward, which needs ceil(A / 4) + 2 passes):
 *   dout            [B,H,W,A] f32   dL/d(out of mr_interpolate_forward)
 *   clip            [B,V,4]   f32   the clip-space vertices the G-buffer was made from
 *   vertex_offsets, vertex_entries  CSR vertex -> (triangle, corner) adjacency of `triangles`
 *                                   (see mr_shade_backward)
 *   dattributes     [B,V,A]   f32 out, dclip [B,V,4] f32 out (16-byte aligned; column z stays 0);
 *                                   both are written completely, no pre-zeroing needed
 *   corner_records  NULL, or the `records` buffer mr_interpolate_forward_records filled for the
 *                   SAME inputs: reused instead of rebuilt
 *   gbuffer_flags   MR_GBUFFER_NORMALISED (see mr_shade_backward): ids / bary are the rasterizer's own
 *                   output for these vertices -- alpha is exactly 1 on every covered pixel, so up to 12
 *                   attributes the pixel pass keeps the 3 A + 9 products in registers down each lane's
 *                   vertical run over difference-basis records (round 4); 0: any G-buffer, general kernels
 * mr_interpolate_forward_records is mr_interpolate_forward for 1 <= A <= that maximum, through
 * per-(image, triangle) corner records (two dependent load levels instead of three; `records`:
 * mr_interpolate_records_bytes(B, T, A) bytes, 256-byte aligned, caller-owned). */
int mr_interpolate_raster_max_attributes(void);
size_t mr_interpolate_records_bytes(int B, int T, int A);

/* rasterize_clip_space()'s forward (src/mesh_renderer/rasterize.py:66-152) for 1 <= A <=
 * mr_interpolate_raster_max_attributes() attributes in ONE pass over the pixels: mr_rasterize_forward with
 * mr_interpolate_forward_records' arithmetic as the epilogue of the tile walk, on the pixel state still in
 * registers (the G-buffer is not read back; the winners' attribute records come from LDS).  Outputs: ids and
 * bary exactly as mr_rasterize_forward writes them, `out` [B,H,W,A] exactly mr_interpolate_forward_records'
 * expression (G-buffer row order), `records` as that call fills them (for mr_interpolate_raster_backward).
 *   z          [B,H,W] f32: scratch -- written only where a crowded region needs it as state between its bin
 *              rounds; undefined afterwards
 *   workspace  mr_rasterize_forward_workspace_bytes() bytes */
int mr_rasterize_interpolate_forward(const float *clip, const float *attrs, const int32_t *triangles,
                                     const float *background, int B, int V, int T, int W, int H, int A,
                                     int32_t *ids, float *bary, float *z, float *out, void *records,
                                     size_t records_bytes, void *workspace, size_t workspace_bytes, void *stream);
int mr_interpolate_forward_records(const int32_t *ids, const float *bary, const float *attrs,
                                   const int32_t *triangles, const float *background, int B, int V,
                                   int T, int W, int H, int A, float *out, void *records,
                                   size_t records_bytes, void *stream);
size_t mr_interpolate_raster_backward_workspace_bytes(int B, int V, int T, int W, int H, int A);
int mr_interpolate_raster_backward(const float *dout, const int32_t *ids, const float *bary,
                                   const float *clip, const float *attributes,
                                   const int32_t *triangles, const float *background,
                                   const int32_t *vertex_offsets, const int32_t *vertex_entries,
                                   const void *corner_records, int B, int V, int T, int W, int H,
                                   int A, float *dattributes, float *dclip, int gbuffer_flags,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* ---- fused deferred shading (diffuse + ambient Phong) ---------------------------
 * Replaces, for render() without specular terms, attribute interpolation
 * (src/mesh_renderer/rasterize.py:118-150), the unpack / normalise / mask block of
 * render() (src/mesh_renderer/render.py:199-215) and phong_shader's ambient +
 * diffuse terms, alpha mask and vertical flip (render.py:287-323, 373-386).
 *   ids, bary                 the G-buffer of mr_rasterize_forward
 *   normals, positions, diffuse  [B,V,3] f32 per-vertex attributes (positions =
 *                             world-space vertices)
 *   light_positions, light_intensities [B,L,3] f32, 1 <= L <= mr_shade_max_lights() (32: the
 *                             reference takes any count, render.py:304-323; up to mr_shade_fast_lights()
 *                             = 4 of them are kept in registers, further ones go through a run-time
 *                             loop).  Two things stay at mr_shade_fast_lights() per call: the specular
 *                             entry points, and light_grads of mr_shade_backward[_l1] -- a caller
 *                             with more lights asks for the light gradients four lights at a time
 *                             (each light's gradient depends on that light alone; see
 *                             pytorch_mesh_renderer_amd/_native.py, shade_backward)
 *   ambient                   [B,3] f32 or NULL
 *   rgba                      [B,H,W,4] f32 out; row 0 is the TOP scanline; alpha is
 *                             1 on covered pixels with a non-negative diffuse colour */
int mr_shade_max_lights(void);
int mr_shade_fast_lights(void);
size_t mr_shade_forward_workspace_bytes(int B, int V, int T, int W, int H);
int mr_shade_forward(const int32_t *ids, const float *bary, const float *normals,
                     const float *positions, const float *diffuse,
                     const int32_t *triangles, const float *light_positions,
                     const float *light_intensities, const float *ambient,
                     int B, int V, int T, int W, int H, int L, float *rgba,
                     void *workspace, size_t workspace_bytes, void *stream);

/* clip[b,v] = transforms[b] . (vertices[b,v], 1): the clip-space transform render() applies before
 * rasterizing (camera_utils.transform_homogeneous, src/common/camera_utils.py:142-170), one thread
 * per vertex; each row is evaluated as ((m0 x + m1 y) + m2 z) + m3 without contraction.
 *   vertices [B,V,3] f32, transforms [B,4,4] f32 row-major (16-byte aligned), clip [B,V,4] f32 out
 *   (16-byte aligned). */
int mr_vertex_transform(const float *vertices, const float *transforms, int B, int V, float *clip,
                        void *stream);

/* render()'s forward from world-space vertices to the image (src/mesh_renderer/render.py:183-228
 * without a specular term): the clip-space transform of camera_utils.transform_homogeneous
 * (src/common/camera_utils.py:142-170), mr_rasterize_forward and mr_shade_forward, the last two in
 * ONE pass over the pixels: the shading runs as the epilogue of the rasterizer's tile walk, on the
 * pixel state still held in registers, so the G-buffer is not read back (and the id ->
 * corner-record gather has one dependent level less).  What FusedPhongRenderer calls.  Outputs:
 * the G-buffer of mr_rasterize_forward run on `clip` (ids, bary, z; bit-identical) and the image
 * of mr_shade_forward (rgba, within the shading's 1e-4 budget).
 *   vertices        [B,V,3] f32  world-space positions (also the shading's `positions`)
 *   transforms      [B,4,4] f32  row-major clip-space transforms, 16-byte aligned
 *   clip            [B,V,4] f32 out  transforms[b] . (vertices[b,v], 1), evaluated per row as
 *                   ((m0 x + m1 y) + m2 z) + m3 without contraction; 16-byte aligned.  The
 *                   backward entry points take it as their `clip` argument.
 *   rgba_u8         NULL, or [B,H,W,4] u8 out (4-byte aligned): the same image as 8-bit frames, exactly
 *                   what mr_export_u8 would make of `rgba` -- for callers that hand frames over or
 *                   write them to files and would otherwise read the float image back (4 B/px of
 *                   stores instead of a 20 B/px pass)
 *   z, want_z       z is always a [B,H,W] buffer; with want_z == 0 the caller declares that it will
 *                   not read it (render() does not): the depth plane is then written only where a
 *                   crowded region needs it as state between its bin rounds, 4 B/px of stores less,
 *                   and its contents after the call are undefined.
 *   corner_records  out, mr_shade_forward_workspace_bytes() bytes, 128-byte aligned: the gathered
 *                   per-triangle attribute records; may be handed to mr_shade_backward.
 *   backward_prepared  NULL, or out: mr_shade_backward_prepared_bytes(B, T) bytes, 256-byte aligned.  For a
 *                   caller that will differentiate the image to the world-space vertices ONLY (the usual
 *                   optimisation loop): the per-triangle setup kernel -- which holds the corner attributes
 *                   and the sign-corrected adjugate in registers anyway -- also writes the records of the
 *                   folded shading backward and clears its accumulator rows.  Handed to
 *                   mr_shade_backward[_l1] as `prepared`, the backward then needs no setup launch.
 *   empty_regions   NULL, or out: mr_empty_regions_bytes(B, W, H) bytes, [B][ceil(H/64)][ceil(W/64)]: 1 = the
 *                   64 x 64-pixel block (G-buffer rows 64 by .. 64 by + 63, i.e. image rows H - 1 - y) is whole and
 *                   holds no candidate triangle: background in the G-buffer, transparent black in the image.
 *                   mr_l1_loss_forward_regions and mr_shade_backward[_l1] skip such blocks without reading them.
 *                   (Launches small enough for 32-pixel regions flag nothing.)
 *   workspace       mr_rasterize_forward_workspace_bytes() bytes */
size_t mr_empty_regions_bytes(int B, int W, int H);
int mr_render_forward(const float *vertices, const float *transforms, const float *normals,
                      const float *diffuse, const int32_t *triangles,
                      const float *light_positions, const float *light_intensities,
                      const float *ambient, int B, int V, int T, int W, int H, int L,
                      float *clip, int32_t *ids, float *bary, float *z, int want_z, float *rgba,
                      uint8_t *rgba_u8, void *corner_records, void *backward_prepared, uint8_t *empty_regions,
                      void *workspace, size_t workspace_bytes, void *stream);

/* mr_render_forward, and mean|rgba - target| out of the same pass: the tile walk's epilogue reads the target's
 * pixel next to the RGBA it is about to store and leaves the loss and its sign codes, so that no loss kernel has to
 * read the image back (16 B/px less, one dependent launch less).  For a FIXED target (an optimisation loop compares
 * every step's image with the same one).  Same arguments and outputs as mr_render_forward, then:
 *   target        [B,H,W,4] f32, 16-byte aligned, image rows like rgba
 *   target_empty  NULL, or the target's block map (mr_image_empty_regions): a region that is empty on both sides
 *                 gets zero codes without its target being read (64-pixel regions only; ignored otherwise)
 *   loss          1 f32 out: sum |rgba - target| / (4 B H W)
 *   signs         [B*H*W] u8 out: one byte of four 2-bit codes per pixel, exactly as mr_l1_loss_forward writes them
 *                 (sign(+-0) = sign(NaN) = 0); what mr_shade_backward_l1 and mr_l1_loss_backward take
 *   partials      scratch, mr_render_forward_l1_partials(B, W, H) floats: one partial sum per region of the
 *                 rasterizer's walk, added in a fixed order by a second, one-workgroup launch: the loss has the
 *                 same bits from run to run.
 * The outputs equal mr_render_forward followed by mr_l1_loss_forward_regions on its image and map, apart from the
 * grouping of the loss's sum (per region instead of per row: equal to a few units of rounding, 1e-6 relative). */
size_t mr_render_forward_l1_partials(int B, int W, int H);
int mr_render_forward_l1(const float *vertices, const float *transforms, const float *normals,
                         const float *diffuse, const int32_t *triangles,
                         const float *light_positions, const float *light_intensities,
                         const float *ambient, int B, int V, int T, int W, int H, int L,
                         float *clip, int32_t *ids, float *bary, float *z, int want_z, float *rgba,
                         uint8_t *rgba_u8, void *corner_records, void *backward_prepared, uint8_t *empty_regions,
                         void *workspace, size_t workspace_bytes, void *stream,
                         const float *target, const uint8_t *target_empty, float *loss, uint8_t *signs,
                         float *partials);

/* mr_render_forward_l1 for a caller that keeps the G-buffer to itself and differentiates the loss to the world-space
 * vertices only (an explicit opt-in: nothing else calls it).  The image, the loss, the sign codes, the partial sums,
 * the empty-region map and the records of `backward_private` have the bits mr_render_forward_l1 gives them.  What
 * differs is the G-buffer, which is PRIVATE to this pair of calls:
 *   - there is no barycentric plane (no `bary` argument; 12 B/px of stores and, in the backward, of loads less);
 *   - ids holds -1, not 0, where nothing was drawn;
 *   - z is scratch (state between the bin rounds of a crowded region), undefined afterwards.
 * Only mr_shade_backward_l1 with MR_GBUFFER_NORMALISED | MR_GBUFFER_PRIVATE reads such a G-buffer: its lane kernel
 * rebuilds a covered pixel's barycentrics from the pixel centre and the triangle's edge functions, with the
 * rasterizer's own un-fused expression and division (the same bits), and tells background by the id.
 *   backward_private  out, mr_render_forward_l1_private_bytes(B, T, W, H) bytes, 256-byte aligned: the block
 *                     mr_render_forward calls backward_prepared, followed by the triangles' edge coefficients and the
 *                     pixel-centre tables.  Handed to mr_shade_backward_l1 as `prepared`; serves ONE backward call. */
size_t mr_render_forward_l1_private_bytes(int B, int T, int W, int H);
int mr_render_forward_l1_private(const float *vertices, const float *transforms, const float *normals,
                                 const float *diffuse, const int32_t *triangles,
                                 const float *light_positions, const float *light_intensities,
                                 const float *ambient, int B, int V, int T, int W, int H, int L,
                                 float *clip, int32_t *ids, float *z, float *rgba, uint8_t *rgba_u8,
                                 void *corner_records, void *backward_private, uint8_t *empty_regions,
                                 void *workspace, size_t workspace_bytes, void *stream,
                                 const float *target, const uint8_t *target_empty, float *loss, uint8_t *signs,
                                 float *partials);

/* Backward of mr_shade_forward AND of the rasterizer underneath it, in one pass
 * over the G-buffer (reads 32 B/px).  All outputs are zeroed here.
 *   drgba        [B,H,W,4] f32  dL/d(rgba); the alpha channel's gradient is ignored
 *   clip         [B,V,4]   f32  the clip-space vertices the G-buffer was made from
 *   dclip        [B,V,4]   f32 out  through the barycentrics (column z stays 0)
 *   dnormals, dpositions, ddiffuse [B,V,3] f32 out  through the interpolated attributes.
 *                               dnormals and / or ddiffuse may be NULL (with the vertex adjacency):
 *                               that gradient is not wanted -- autograd's needs_input_grad -- and its
 *                               nine sums per triangle are not formed; without light_grads the pixel
 *                               pass then keeps the 18 or 27 remaining products in registers down each
 *                               lane's vertical run (k_accumulate_lanes) instead of reducing 36 per row
 *   light_grads  [B, 6L+3] f32 out  per image: d light_positions (L x 3),
 *                               d light_intensities (L x 3), d ambient (3; 0 if NULL).
 *                               NULL: not wanted -- an instantiation without the nine per-lane
 *                               accumulators runs (the pixel pass 4 % faster)
 *   corner_records  NULL, or the first mr_shade_forward_workspace_bytes() bytes of the workspace
 *                   mr_shade_forward ran with for the SAME inputs (128-byte aligned): its gathered
 *                   per-triangle attribute records are then reused instead of rebuilt.
 *   vertex_offsets, vertex_entries  both NULL, or the CSR vertex -> (triangle, corner) adjacency of
 *                   `triangles`: offsets [V+1] i32, entries [offsets[V]] i32 with entry = 3 *
 *                   triangle + corner, grouped by vertex (corners whose index is outside [0, V)
 *                   left out).  With it the per-triangle sums are GATHERED per vertex (no atomics,
 *                   fixed summation order); without it they are scattered with float atomics.
 *   transforms      NULL, or the [B,4,4] row-major clip-space transforms that `clip` was made with
 *                   (clip = transforms . (positions, 1), as mr_render_forward does): dpositions then
 *                   also receives the clip-space gradient pulled back through that product, i.e.
 *                   it becomes the whole gradient w.r.t. the world-space vertices; dclip is still
 *                   written (a caller that differentiates the transforms needs it).  Requires the
 *                   vertex adjacency.  With transforms, dclip may be NULL: the clip-space gradient is
 *                   not wanted on its own (the caller differentiates to the vertices, not to the
 *                   cameras).  Where the lane kernel has the variant (no light_grads, dnormals and
 *                   ddiffuse NULL, MR_GBUFFER_NORMALISED, not deterministic) the pull-back is then applied
 *                   per pixel and the pixel pass keeps 9 sums per triangle instead of 18; elsewhere the
 *                   clip gradient goes to the workspace.
 *   prepared        NULL, or the block mr_render_forward filled as `backward_prepared` for the SAME
 *                   inputs (256-byte aligned).  Used -- the setup launch skipped -- when the call is one
 *                   the folded kernel serves (dclip, dnormals, ddiffuse, light_grads NULL; transforms and
 *                   the adjacency given; MR_GBUFFER_NORMALISED; not deterministic), ignored otherwise.  The
 *                   block's accumulator rows are clear on entry and DIRTY afterwards: a block serves ONE
 *                   backward call that uses it (differentiating a second time: pass NULL -- the call then
 *                   runs its own setup kernel -- or clear the rows, the block's last
 *                   B * T * 48 bytes rounded up to 256).
 *   empty_regions   NULL, or mr_render_forward's `empty_regions` for the SAME G-buffer: the difference-basis lane
 *                   kernels leave a strip that lies inside an empty block without reading it.
 * dclip, dnormals, dpositions, ddiffuse, light_grads laid out back to back in that order are
 * zeroed with a single memset (none at all with the vertex adjacency: every output is written
 * exactly once). */
size_t mr_shade_backward_prepared_bytes(int B, int T);
size_t mr_shade_backward_workspace_bytes(int B, int V, int T, int W, int H);
int mr_shade_backward(const float *drgba, const int32_t *ids, const float *bary,
                      const float *clip, const float *normals, const float *positions,
                      const float *diffuse, const int32_t *triangles,
                      const float *light_positions, const float *light_intensities,
                      const float *ambient, int B, int V, int T, int W, int H, int L,
                      float *dclip, float *dnormals, float *dpositions,
                      float *ddiffuse, float *light_grads, const void *corner_records,
                      const int32_t *vertex_offsets, const int32_t *vertex_entries,
                      const float *transforms, int gbuffer_flags, void *prepared, const uint8_t *empty_regions,
                      void *workspace, size_t workspace_bytes,
                      void *stream);
/* gbuffer_flags, bit 0 = MR_GBUFFER_NORMALISED: the caller vouches that ids / bary are what
 * mr_rasterize_forward (or mr_render_forward) wrote for these very vertices -- every covered pixel's
 * barycentrics sum to 1 within rounding.  The coverage alpha = clamp(2 * sum) (rasterize.py:137-150) is then
 * exactly 1 and outside the clamp's pass band, and the pixel pass leaves out the blend with the background
 * and the d / d alpha terms: the same bits with ~20 % fewer vector instructions per pixel.  0 = any
 * G-buffer (e.g. one the caller edited). */
#define MR_GBUFFER_NORMALISED 1
/* bit 1 = MR_GBUFFER_PRIVATE (mr_shade_backward_l1 only, together with MR_GBUFFER_NORMALISED): ids is the private id
 * plane of mr_render_forward_l1_private (-1 = nothing drawn), `bary` is not read (NULL will do) and `prepared` is
 * that call's backward_private block.  Vertex gradients only (dnormals, ddiffuse, dclip, light_grads NULL;
 * transforms, corner_records and the adjacency given), one to four lights, not deterministic: MR_EINVAL otherwise. */
#define MR_GBUFFER_PRIVATE 2

/* mr_shade_backward for an upstream gradient that is the backward of mr_l1_loss_forward(rgba,
 * target): instead of the [B,H,W,4] float image mr_l1_loss_backward would write (16 B/px) it takes
 * the loss's packed sign codes (`signs`, one byte per pixel in image row order, exactly as
 * mr_l1_loss_forward wrote them for an image of B*H*W*4 elements) and `upstream`, the device scalar
 * d L / d loss.  Same outputs as mr_shade_backward(drgba = upstream * sign / (B*H*W*4)); the
 * workspace must be mr_shade_backward_l1_workspace_bytes() long. */
size_t mr_shade_backward_l1_workspace_bytes(int B, int V, int T, int W, int H);
int mr_shade_backward_l1(const uint8_t *signs, const float *upstream, const int32_t *ids,
                         const float *bary, const float *clip, const float *normals,
                         const float *positions, const float *diffuse, const int32_t *triangles,
                         const float *light_positions, const float *light_intensities,
                         const float *ambient, int B, int V, int T, int W, int H, int L,
                         float *dclip, float *dnormals, float *dpositions, float *ddiffuse,
                         float *light_grads, const void *corner_records,
                         const int32_t *vertex_offsets, const int32_t *vertex_entries,
                         const float *transforms, int gbuffer_flags, void *prepared, const uint8_t *empty_regions,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---- fused deferred shading with the specular term --------------------------------
 * The same replacement as mr_shade_forward / mr_shade_backward for render() calls that pass
 * specular_colors and shininess_coefficients (src/mesh_renderer/render.py:157-181, 199-228;
 * phong_shader's specular term :326-372, including its L2 normalisation of the reflection .
 * camera dot product ACROSS ALL PIXELS of an image, :342-348 -- one extra pass over the
 * G-buffer each way).  Additional arguments:
 *   specular         [B,V,3] f32  per-vertex specular colours
 *   camera_position  [B,3]   f32  world-space eye
 *   shininess        [B] f32 one exponent per image, or, with shininess_per_vertex != 0,
 *                    [B,V] f32 one per vertex (interpolated as a 13th attribute, render.py
 *                                 :171-181, 222-224)
 *   norms2           [B,L]   f32  forward: out, sum over all pixels of (reflection . camera)^2;
 *                                 backward: in, the forward's values
 *   dspecular        [B,V,3] f32 out
 *   dshininess       [B,V]   f32 out  d per-vertex shininess; used (and required) only with
 *                                 shininess_per_vertex != 0
 *   light_grads      [B, 6L+7] f32 out  per image: d light_positions (L x 3), d light_intensities
 *                                 (L x 3), d ambient (3; 0 if NULL), d camera_position (3),
 *                                 d per-image shininess (1; 0 with per-vertex exponents)
 *   vertex_offsets, vertex_entries (backward)  both NULL, or the CSR vertex adjacency of `triangles`
 *                                 exactly as for mr_shade_backward: the per-triangle sums are then
 *                                 gathered per vertex (no atomics, every output written once, fixed
 *                                 order) instead of scattered with float atomics; required in the
 *                                 deterministic mode
 *   transforms, gbuffer_flags, grads_wanted (backward, round 4)
 *                                 grads_wanted: MR_GRAD_* bits of the gradients the caller will read; an
 *                                 output whose bit is clear still has to be a valid buffer and holds
 *                                 unspecified values afterwards (MR_GRAD_ALL: everything, as before).
 *                                 When only MR_GRAD_POSITIONS / MR_GRAD_CLIP are wanted -- render()
 *                                 differentiated to the vertices alone -- and gbuffer_flags has
 *                                 MR_GBUFFER_NORMALISED (see mr_shade_backward) and the deterministic mode is
 *                                 off, the pixel pass keeps its 18 sums per triangle in registers down each
 *                                 lane's vertical run instead of reducing 45 through LDS per pixel
 *                                 (0.64 -> 0.3x ms at 1024^2 x 32).  transforms ([B,4,4], clip = M (position,
 *                                 1)) or NULL: with them and MR_GRAD_CLIP clear the pull-back M^T dclip is
 *                                 folded into dpositions, which is then the whole gradient w.r.t. the
 *                                 world-space vertices (9 sums).
 * Only pixels that pass render()'s mask (render.py:215) evaluate the power; the reference's
 * autograd multiplies the masked pixels' zero gradient by pow(0, -1) = inf of the background
 * exponent -1 and returns NaN for every per-vertex-shininess call with a background pixel. */
#define MR_GRAD_NORMALS 1
#define MR_GRAD_POSITIONS 2
#define MR_GRAD_DIFFUSE 4
#define MR_GRAD_SPECULAR 8
#define MR_GRAD_SHININESS 16   /* per-vertex (dshininess) or per-image (light_grads' last column) */
#define MR_GRAD_LIGHTS 32      /* light_grads: light positions / intensities, ambient, camera position */
#define MR_GRAD_CLIP 64
#define MR_GRAD_ALL 127
size_t mr_shade_specular_forward_workspace_bytes(int B, int V, int T, int W, int H);
int mr_shade_specular_forward(const int32_t *ids, const float *bary, const float *normals,
                              const float *positions, const float *diffuse, const float *specular,
                              const int32_t *triangles, const float *light_positions,
                              const float *light_intensities, const float *ambient,
                              const float *camera_position, const float *shininess,
                              int shininess_per_vertex, int B, int V, int T, int W, int H, int L,
                              float *rgba, float *norms2, int norms2_given,
                              void *workspace, size_t workspace_bytes, void *stream);
/* norms2_given = 1: norms2 is an INPUT -- what mr_rasterize_specular_norms_forward wrote for the same G-buffer, normals,
 * positions, lights and camera -- and the norm pass over the G-buffer does not run (0: norms2 is an output, as before).
 *
 * mr_rasterize_specular_norms_forward (round 5): mr_rasterize_forward on `clip` AND those norms in one pass over the
 * pixels.  The reference L2-normalises the reflection . camera dot product across ALL pixels of an image per light
 * (render.py:342-348); that sum only needs every covered pixel's interpolated normal and position, which the
 * rasterizer's tile walk holds when it has settled the pixel, and the uncovered pixels all carry the background's
 * attributes -1 (render.py:197) and one common value.  ids / bary / z exactly as mr_rasterize_forward writes them (z is
 * required as a buffer; want_z = 0: its contents are unspecified afterwards); norms2 [B,L] f32 out, 1 <= L <= 4. */
size_t mr_rasterize_specular_norms_workspace_bytes(int B, int V, int T, int W, int H);
int mr_rasterize_specular_norms_forward(const float *clip, const int32_t *triangles, const float *normals,
                                        const float *positions, const float *light_positions,
                                        const float *camera_position, int B, int V, int T, int W, int H, int L,
                                        int32_t *ids, float *bary, float *z, int want_z, float *norms2,
                                        void *workspace, size_t workspace_bytes, void *stream);
size_t mr_shade_specular_backward_workspace_bytes(int B, int V, int T, int W, int H);
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
                               int grads_wanted, void *workspace, size_t workspace_bytes, void *stream);
/* mr_shade_specular_backward for an upstream gradient that is the backward of mr_l1_loss_forward(rgba, target)
 * -- the reference's optimisation loop, mesh_renderer_test.py:238-262, on the specular renderer (render.py:224-246):
 * `signs` / `upstream` as in mr_shade_backward_l1, in place of drgba.  Same outputs as
 * mr_shade_specular_backward(drgba = upstream * sign / (B*H*W*4)).  The one-pass vertex-gradient kernel (one or two
 * lights, transforms given, only MR_GRAD_POSITIONS wanted, MR_GBUFFER_NORMALISED, adjacency given, deterministic mode
 * off) reads the codes directly, 1 B/px instead of 16; every other case writes the dense image into the workspace
 * first and runs mr_shade_specular_backward's kernels.  The workspace must be
 * mr_shade_specular_backward_l1_workspace_bytes() long. */
size_t mr_shade_specular_backward_l1_workspace_bytes(int B, int V, int T, int W, int H);
int mr_shade_specular_backward_l1(const uint8_t *signs, const float *upstream, const int32_t *ids,
                                  const float *bary, const float *clip, const float *normals,
                                  const float *positions, const float *diffuse, const float *specular,
                                  const int32_t *triangles, const float *light_positions,
                                  const float *light_intensities, const float *ambient,
                                  const float *camera_position, const float *shininess,
                                  int shininess_per_vertex, const float *norms2, int B, int V, int T,
                                  int W, int H, int L, float *dclip, float *dnormals, float *dpositions,
                                  float *ddiffuse, float *dspecular, float *dshininess,
                                  float *light_grads, const int32_t *vertex_offsets,
                                  const int32_t *vertex_entries, const float *transforms, int gbuffer_flags,
                                  int grads_wanted, void *workspace, size_t workspace_bytes, void *stream);

/* ---- SoftRas renderer ---------------------------------------------------------------
 * Replaces rasterize_batch / rasterize of the reference's second renderer
 * (src/soft_mesh_renderer/rasterize.py:14-110, 212-424) and the autograd graph behind it.
 *   clip               [B,V,4] f32   clip-space vertices
 *   positions, normals, diffuse [B,V,3] f32 (positions = world-space vertices)
 *   triangles          [T,3] i32     counter-clockwise = front-facing (back faces are culled)
 *   light_positions    [B,L,3] f32, light_intensities [B,L] f32 (scalar), 1 <= L <= mr_soft_max_lights()
 *   sigma, gamma, blur the reference's sigma_val, gamma_val, blur_radius (NDC units)
 *   rgba               [B,H,W,4] f32 out; row 0 is the TOP scanline; alpha = silhouette
 *   aux                [B,H,W,4] f32 out; per-pixel softmax state kept for the backward */
int mr_soft_max_lights(void);
size_t mr_soft_workspace_bytes(int B, int V, int T, int W, int H);
int mr_soft_forward(const float *clip, const float *positions, const float *normals,
                    const float *diffuse, const int32_t *triangles,
                    const float *light_positions, const float *light_intensities,
                    int B, int V, int T, int W, int H, int L,
                    float sigma, float gamma, float blur, float *rgba, float *aux,
                    void *workspace, size_t workspace_bytes, void *stream);
/* mr_soft_forward leaves its per-triangle records and candidate lists in the first
 * mr_soft_prepared_bytes() of its workspace.  A caller that keeps that workspace untouched until the
 * backward pass of the SAME inputs and sizes hands it over as `prepared` and the backward does not
 * rebuild them (three launches); prepared = NULL rebuilds them in `workspace`.  The forward itself is
 * content with a workspace of mr_soft_prepared_bytes(); the backward wants mr_soft_workspace_bytes(). */
size_t mr_soft_prepared_bytes(int B, int V, int T, int W, int H);
/* All gradient outputs are zeroed here.  drgba [B,H,W,4]; dclip [B,V,4];
 * dpositions / dnormals / ddiffuse [B,V,3]; dlight_positions [B,L,3]; dlight_intensities [B,L]. */
int mr_soft_backward(const float *drgba, const float *rgba, const float *aux,
                     const float *clip, const float *positions, const float *normals,
                     const float *diffuse, const int32_t *triangles,
                     const float *light_positions, const float *light_intensities,
                     int B, int V, int T, int W, int H, int L,
                     float sigma, float gamma, float blur,
                     float *dclip, float *dpositions, float *dnormals, float *ddiffuse,
                     float *dlight_positions, float *dlight_intensities, const void *prepared,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---- mean-absolute-error image loss --------------------------------------------------
 * The loss the reference's optimisation tests and examples use,
 * torch.mean(torch.abs(render - target)) (src/mesh_renderer/mesh_renderer_test.py:250),
 * as one streaming pass each way.  a, b: n floats (16-byte aligned); loss: 1 float out;
 * signs: (n + 3) / 4 bytes out, or NULL when no gradient is wanted -- byte i holds
 * sign(a - b) of elements 4i .. 4i+3 as 2-bit two's-complement codes (0: zero, 1: +1, 3: -1), so that the
 * backward pass does not read the images again; upstream: 1 float (dL/dloss, read on the
 * device); da: n floats out (16-byte aligned) = upstream * sign(a - b) / n.
 * partials: MR_L1_PARTIALS floats of scratch: the workgroups' partial sums, added in a fixed
 * order by one wavefront -- the loss value is bit-identical from run to run. */
#define MR_L1_PARTIALS 2048
/* The same loss for [B,H,W,4] images whose EMPTY 64 x 64 blocks are known (round 4): empty_a / empty_b are
 * mr_empty_regions_bytes(B, W, H) byte maps as mr_render_forward writes them for its image and
 * mr_image_empty_regions computes them for any image (once per target).  Where both say 1 the block is neither read
 * nor compared -- |0 - 0| = 0, sign codes 0 -- which for an object over an empty background is the share of the
 * frame it leaves free.  Same loss value up to the grouping of the sum (still a fixed order), same sign codes. */
int mr_image_empty_regions(const float *image, int B, int H, int W, uint8_t *map, void *stream);
int mr_l1_loss_forward_regions(const float *a, const float *b, int B, int H, int W, const uint8_t *empty_a,
                               const uint8_t *empty_b, float *loss, uint8_t *signs, float *partials, void *stream);
int mr_l1_loss_partials(void); /* MR_L1_PARTIALS of the library that was loaded (a binding without the header asks) */
int mr_l1_loss_forward(const float *a, const float *b, size_t n, float *loss, uint8_t *signs,
                       float *partials, void *stream);
int mr_l1_loss_backward(const uint8_t *signs, size_t n, const float *upstream, float *da,
                        void *stream);

/* ---- structural-similarity image loss (no reference counterpart) ----------------------------
 * The mean SSIM (Wang et al. 2004) of two images ("Image losses: SSIM"), one stencil pass each way.
 * Channels are independent.  Window g[i] ~ exp(-(i - r)^2 / (2 sigma^2)), i = 0 .. window - 1, r = (window - 1) / 2,
 * normalised to sum 1 in double and rounded to float on the host inside the library; G = g x g.  Per channel and pixel
 *   mx = G*x  my = G*y  sxx = G*(x x) - mx^2  syy = G*(y y) - my^2  sxy = G*(x y) - mx my
 *   map = ((2 mx my + c1)(2 sxy + c2)) / ((mx^2 + my^2 + c1)(sxx + syy + c2))
 * MR_SSIM_SAME: taps outside the image contribute zero, the weights are not renormalised, the map is [B,H,W,C]
 * (conv2d with padding window / 2); MR_SSIM_VALID: only windows wholly inside, the map is
 * [B,H-window+1,W-window+1,C] and H, W >= window.  The value is the plain mean of the map.
 *   image, target [B,H,W,C] f32, 1 <= C <= 4; every pointer 16-byte aligned when C = 4
 *   window        odd, 3 .. 11;  sigma > 0;  c1, c2 > 0: (k1 L)^2 and (k2 L)^2 (with 0 the map would be 0 / 0 where
 *                 both images are flat)
 *   grads         mask of MR_SSIM_GRAD_*: which input the backward will differentiate
 *   mean          1 float out (device)
 *   map           the map out, or NULL (not written)
 *   saved         mr_ssim_saved_floats() floats out, needed unless grads is 0: planes of the map's shape that the
 *                 backward convolves, each already times 1 / n -- with the map f as a function of the raw moments
 *                 (mx, my, Exx, Eyy, Exy): d f / d Exx (= d f / d Eyy), d f / d Exy, then d f / d mx if the image is
 *                 in grads, then d f / d my if the target is
 *   partials      scratch, mr_ssim_partials() floats: one partial sum per workgroup (a 32 x 16 tile of the map), added
 *                 in a fixed order by a second launch -- the value is bit-identical from run to run
 * Backward: upstream (1 float, d L / d mean, read on the device) -> dimage and / or dtarget [B,H,W,C], either may be
 * NULL (not computed), each only if the forward's grads named it (same grads in both calls):
 *   d L / d x(q) = upstream ((G*A)(q) + 2 x(q) (G*B)(q) + y(q) (G*C)(q))
 * with A, B, C the planes d f / d mx, d f / d Exx, d f / d Exy (zero outside the map).  A gather with no atomics:
 * bit-reproducible in either deterministic mode.  Both calls are asynchronous on `stream`, allocate nothing and do
 * not synchronise.  1 <= B <= 65535, H, W <= 65535, B H W < 2^36; anything else is MR_EINVAL before any device
 * call, and the size queries return 0. */
#define MR_SSIM_SAME 0
#define MR_SSIM_VALID 1
#define MR_SSIM_GRAD_IMAGE 1
#define MR_SSIM_GRAD_TARGET 2
size_t mr_ssim_partials(int B, int H, int W, int window, int padding);
size_t mr_ssim_saved_floats(int B, int H, int W, int C, int window, int padding, int grads);
int mr_ssim_forward(const float *image, const float *target, int B, int H, int W, int C, int window, float sigma,
                    float c1, float c2, int padding, int grads, float *mean, float *map, float *saved, float *partials,
                    void *stream);
int mr_ssim_backward(const float *image, const float *target, const float *saved, const float *upstream, int B, int H,
                     int W, int C, int window, float sigma, int padding, int grads, float *dimage, float *dtarget,
                     void *stream);

/* ---- 8-bit frame export ---------------------------------------------------------------
 * The conversion the reference's examples apply on the host before writing PNG / GIF frames,
 * (image * 255.0).astype(np.uint8) (src/examples/example1.py:52, example5.py:81), on the device:
 * out[i] = (uint8) trunc(clamp(image[i], 0, 1) * 255), NaN -> 0.  image: n floats (16-byte
 * aligned); out: n bytes (4-byte aligned).  Used for frames that leave the GPU (display, files,
 * the multi-GPU hand-over): a quarter of the fp32 bytes. */
int mr_export_u8(const float *image, size_t n, uint8_t *out, void *stream);

/* ---- vertex normals ---------------------------------------------------------------------
 * Replaces compute_vertex_normals (src/common/meshes.py:3-35): for every triangle corner the
 * area-weighted face normal (next - this) x (next_next - this) is added to the corner's vertex and
 * the sums are normalised (eps 1e-6).  Gather form over the CSR vertex -> (triangle, corner)
 * adjacency of `triangles` (vertex_offsets [V+1], vertex_entries, entry = 3 * triangle + corner,
 * see mr_shade_backward): no atomics, fixed summation order.  Triangles with a vertex id outside
 * [0, V) are skipped.
 *   vertices [B,V,3] f32;  sums [B,V,3] f32 out (the un-normalised sums, input of the backward);
 *   normals [B,V,3] f32 out;  backward: dnormals in, dvertices [B,V,3] out. */
int mr_vertex_normals_forward(const float *vertices, const int32_t *triangles,
                              const int32_t *vertex_offsets, const int32_t *vertex_entries, int B, int V,
                              int T, float *sums, float *normals, void *stream);
int mr_vertex_normals_backward(const float *dnormals, const float *vertices, const float *sums,
                               const int32_t *triangles, const int32_t *vertex_offsets,
                               const int32_t *vertex_entries, int B, int V, int T, float *dvertices,
                               void *stream);

/* ---- silhouette antialiasing (no reference counterpart) ----------------------------------
 * Analytic antialiasing of a hard-rasterized image ("Silhouette antialiasing"): each
 * horizontal / vertical pair of neighbouring pixels whose ids differ, or of which exactly one is covered
 * (id != 0 or (b0 + b1) + b2 >= 0.9), is blended by where the front triangle's exit edge crosses the
 * segment between the two pixel centres, when that edge is a silhouette of the mesh; the crossing point is
 * differentiated with respect to the edge's clip-space x, y, w.  Decisions in un-fused binary32.
 *   image     [B,H,W,C] f32, any C >= 1, rows in the rasterizer's order (row 0 = bottom)
 *   ids, bary, z  [B,H,W] i32, [B,H,W,3] f32, [B,H,W] f32: mr_rasterize_forward's outputs for `clip`
 *   clip      [B,V,4] f32, 16-byte aligned
 *   triangles [T,3] i32, shared by the batch
 *   opposite  [T,3] i32: for the edge opposite corner k of triangle t, the neighbouring triangle's vertex
 *             across it, -1 for a boundary edge, -2 for a non-manifold or degenerate one
 *             (mesh_renderer.antialias_topology)
 *   out       [B,H,W,C] f32 out (may not alias image); image 16-byte aligned when C = 4
 *   pair_mask [B,H,W] u8 out, optional (NULL = not written): bit k (left, right, down, up) set where the
 *             pair of this pixel and that neighbour blended and modified THIS pixel
 * Backward: dout [B,H,W,C] -> dimage [B,H,W,C] (gather form, no atomics) and dclip [B,V,4] (zeroed by the
 * callee; column z stays 0).  dclip is summed with float atomics, or in 64-bit fixed point under
 * mr_set_deterministic(1), which needs the workspace. */
int mr_antialias_forward(const float *image, const int32_t *ids, const float *bary, const float *z,
                         const float *clip, const int32_t *triangles, const int32_t *opposite, int B, int V,
                         int T, int W, int H, int C, float *out, uint8_t *pair_mask, void *stream);
size_t mr_antialias_backward_workspace_bytes(int B, int V, int T, int W, int H, int C);
int mr_antialias_backward(const float *dout, const float *image, const int32_t *ids, const float *bary,
                          const float *z, const float *clip, const int32_t *triangles, const int32_t *opposite,
                          int B, int V, int T, int W, int H, int C, float *dimage, float *dclip, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ---- spherical-harmonics lighting (no reference counterpart) ------------------------------
 * Diffuse shading of a pixel buffer under second-order SH irradiance ("Spherical-harmonics
 * lighting"): n = N / max(|N|, 1e-12), E_c = sum_k sh[b,k,c] Y_k(n) with no clamp, rgb = diffuse * E, rgb = 0
 * where alpha <= 0.5, RGBA out.
 *   normals, diffuse  pixel i of the batch at normals + i * pixel_stride, diffuse + i * pixel_stride (3 floats
 *             each): two [B,H,W,3] buffers (pixel_stride 3) or two channel slices of one [B,H,W,C] buffer
 *             (pixel_stride C >= 3), pixels in the rasterizer's order
 *   alphas    [B,H,W] f32, or NULL: alpha = 1 where any diffuse channel is >= 0, else 0 (background = -1)
 *   sh        [B,9,3] f32: world-space irradiance coefficients, basis k, channel c
 *   flip      nonzero: output row H-1-y holds input row y (row 0 = top, as render()); zero: the same row order
 *   rgba      [B,H,W,4] f32 out, 16-byte aligned
 * B <= 65535 and W * H <= 2^30.
 * Backward: drgba [B,H,W,4] (16-byte aligned, rows as rgba) -> dnormals, ddiffuse (pixel_stride as the inputs),
 * dalphas [B,H,W] (the alpha channel of drgba; only with alphas) and dsh [B,9,3].  Each of the four may be NULL
 * (not wanted).  Gather form, no atomics: every pixel writes its own gradients (zeros where masked); dsh is summed
 * per workgroup into the workspace (needed only with dsh) and then in a fixed order, so it is bit-reproducible. */
int mr_sh_shade_forward(const float *normals, const float *diffuse, int pixel_stride, const float *alphas,
                        const float *sh, int B, int W, int H, int flip, float *rgba, void *stream);
size_t mr_sh_shade_backward_workspace_bytes(int B, int W, int H);
int mr_sh_shade_backward(const float *drgba, const float *normals, const float *diffuse, int pixel_stride,
                         const float *alphas, const float *sh, int B, int W, int H, int flip, float *dnormals,
                         float *ddiffuse, float *dalphas, float *dsh, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ---- bilinear texture mapping (no reference counterpart) ---------------------------------
 * Samples a texture at a pixel buffer of UV coordinates ("Texture mapping"), with the
 * conventions of grid_sample(align_corners=False): texel (i, j) covers u in [j/Wt, (j+1)/Wt) and v in
 * [i/Ht, (i+1)/Ht), row 0 is v = 0.  x = fl(fl(u * Wt) - 0.5f), y likewise (binary32, un-fused), x0 = floor(x),
 * fx = x - x0; the value is the bilinear blend of the taps (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1), their indices
 * wrapped (MR_TEXTURE_WRAP) or clamped to the edge (MR_TEXTURE_CLAMP).  A pixel is 0 in every channel, and passes
 * no gradient, where mask <= 0.5, where u or v is not finite, or where |x| or |y| >= 2^24.
 *   tex         [Ht,Wt,C] (tex_batched 0: shared by every image) or [B,Ht,Wt,C] (tex_batched 1) f32, 1 <= C <= 4
 *   uv          [B,H,W,2] f32;  mask [B,H,W] f32 or NULL
 *   out         [B,H,W,C] f32
 * tex, out, dout and dtex 16-byte aligned, uv and duv 8-byte aligned.  B <= 65535, W * H <= 2^30,
 * ceil(W / 64) * ceil(H / 16) <= 2^22 (the backward's 64 x 16 pixel tiles: only very thin images are refused),
 * Ht, Wt <= 65536, Ht * Wt <= 2^28.
 * Backward: dout [B,H,W,C] -> dtex (tex's shape; a shared texture sums over the batch) and duv [B,H,W,2], each
 * optional (NULL = not wanted).  duv is written per pixel (0 where skipped) and is reproducible in either mode.
 * dtex is a scatter: float atomics, or 64-bit fixed point under mr_set_deterministic(1), which needs the
 * workspace (mr_texture_backward_workspace_bytes reports the need of the calling thread's current mode: 0
 * in float mode). */
#define MR_TEXTURE_WRAP 0
#define MR_TEXTURE_CLAMP 1
int mr_texture_forward(const float *tex, const float *uv, const float *mask, int tex_batched, int Ht, int Wt, int C,
                       int B, int W, int H, int boundary, float *out, void *stream);
size_t mr_texture_backward_workspace_bytes(int tex_batched, int Ht, int Wt, int C, int B, int W, int H);
int mr_texture_backward(const float *dout, const float *tex, const float *uv, const float *mask, int tex_batched,
                        int Ht, int Wt, int C, int B, int W, int H, int boundary, float *dtex, float *duv,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ---- mipmapped trilinear texture mapping (no reference counterpart) ----------------------
 * The same lookup, prefiltered ("Texture mapping").  Pyramid: level 0 is tex; level l + 1 exists
 * while both extents of level l are even, L = 1 + min(tz(Ht), tz(Wt), max_level) levels (tz: trailing zero bits;
 * max_level < 0: no cap; L <= 17), its texel fl(fl(fl(a + b) + fl(c + d)) * 0.25f) of the 2 x 2 block (2i,2j)
 * (2i,2j+1) (2i+1,2j) (2i+1,2j+1) below, per channel; one pyramid per image for a batched texture.
 * mr_texture_mip_levels reports L (0 for extents outside 1 .. 65536).
 *   uv_da       [B,H,W,4] f32, 16-byte aligned: (du/dX, du/dY, dv/dX, dv/dY) per step of one output pixel
 *   pyramid     levels >= 1, packed, mr_texture_mip_pyramid_bytes() bytes, 16-byte aligned (may be NULL when that
 *               is 0): written by the forward, read by the backward
 * ax^2 = (du/dX Wt)^2 + (dv/dX Ht)^2, ay^2 likewise with d/dY, lod = 0.5f * log2f(max(ax^2, ay^2)), 0 when a
 * derivative is NaN, clamped to [0, L - 1]; l0 = floor(lod), f = lod - l0.  The value is the bilinear rule above at
 * level l0 with that level's extents, and, when f > 0, (1 - f) times it plus f times the same at level l0 + 1.  The
 * skip rule is the bilinear one, evaluated at level 0.  With uv_da all zero the output equals mr_texture_forward's
 * bit for bit.
 * Backward: duv is the level-weighted sum of the two levels' bilinear derivatives; dtex scatters (level weight x tap
 * weight x dout) into a gradient pyramid (float atomics, or 64-bit fixed point under mr_set_deterministic(1)) and
 * folds it coarsest level first, dlevel_l[i,j] += 0.25f dlevel_{l+1}[i/2,j/2], gathered; level 0 is dtex.  uv_da and
 * mask get no gradient.  The workspace (gradient pyramid; fixed-point copy) is needed whenever dtex is wanted. */
int mr_texture_mip_levels(int Ht, int Wt, int max_level);
size_t mr_texture_mip_pyramid_bytes(int tex_batched, int Ht, int Wt, int C, int B, int max_level);
int mr_texture_mip_forward(const float *tex, const float *uv, const float *uv_da, const float *mask, int tex_batched,
                           int Ht, int Wt, int C, int B, int W, int H, int boundary, int max_level, float *pyramid,
                           float *out, void *stream);
size_t mr_texture_mip_backward_workspace_bytes(int tex_batched, int Ht, int Wt, int C, int B, int W, int H,
                                               int max_level);
int mr_texture_mip_backward(const float *dout, const float *tex, const float *pyramid, const float *uv,
                            const float *uv_da, const float *mask, int tex_batched, int Ht, int Wt, int C, int B,
                            int W, int H, int boundary, int max_level, float *dtex, float *duv, void *workspace,
                            size_t workspace_bytes, void *stream);

/* ---- screen-space attribute derivatives (forward only) -----------------------------------
 * out [B,H,W,A,2] f32 (8-byte aligned), 1 <= A <= 4: (d a / d X, d a / d Y) of the perspective-correct
 * interpolation of attributes [B,Va,A] per step of one pixel column (X) / row (Y) of the G-buffer, from the
 * rasterizer's edge functions: with b_i = e_i / s, e_i = U[3i] px + U[3i+1] py + U[3i+2], s = e0 + e1 + e2,
 *   d a / d X = (2 / W) sum_i a_i (U[3i] - b_i (U[0] + U[3] + U[6])) / s      (d / d Y: U[3i+1], 2 / H).
 * Corner values are read through attribute_triangles [T,3] when given (per-corner attributes), else through
 * triangles (then Va = V).  Background pixels (sum of barycentrics not positive) are 0.  clip 16-byte aligned.
 * For A = 2 the output viewed as [B,H,W,4] is mr_texture_mip_forward's uv_da. */
int mr_attribute_derivatives(const int32_t *ids, const float *bary, const float *clip, const int32_t *triangles,
                             const float *attributes, const int32_t *attribute_triangles, int B, int V, int T,
                             int Va, int W, int H, int A, float *out, void *stream);

/* ---- mesh regularisers (no reference counterpart in the library; the reference's example7b.py has two) ----
 * Uniform Laplacian, edge length and normal consistency of a batch of meshes that share one topology
 * ("Mesh regularisers"), per image b:
 *   lap  = 1/V sum_i |delta_i|,  delta_i = 1/deg_i sum_{j in N(i)} v_j - v_i   (0 for a vertex without neighbours)
 *   edge = 1/E sum_e |v_lo - v_hi|   (use_target 0)   or   1/E sum_e (|v_lo - v_hi| - target_length)^2   (nonzero)
 *   nc   = 1/F sum_flaps (1 - cos(n0, n1)),  n0 = (b-a) x (c-a),  n1 = (d-a) x (b-a);  a flap with |n0| <= 1e-8 or
 *          |n1| <= 1e-8 has value 0 and gradient 0 and still counts in F
 * A zero delta_i and a zero-length edge have gradient 0; E = 0 and F = 0 give 0.
 *   vertices     [B,V,3] f32
 *   nbr_offsets  [V+1] i32, nbr [2E] i32: CSR of every vertex's neighbours (each undirected edge appears at both
 *                ends; an edge is counted at the end with the lower index)
 *   flaps        [F,4] i32 (a, b, c, d): one row per edge (a, b) shared by exactly two triangles, c and d the
 *                opposite corners
 *   role_offsets [V+1] i32, roles [4F] i32: CSR of every vertex's (flap, role) pairs, entry = 4 * flap + role
 *                (role 0..3 = a..d); the backward only
 *   terms        bit mask of MR_MESH_*: a term that is not asked for is not computed and reads 0
 *   unit_dirs    [B,V,3] f32: delta_i / |delta_i| (0 where delta_i = 0), written by the forward and read by the
 *                backward; needed with MR_MESH_LAPLACIAN only
 *   out_terms    [B,3] f32 out: (lap, edge, nc)
 *   dterms       [B,3] f32 (device);  dvertices [B,V,3] f32 out, written completely
 * 1 <= B <= 65535, 1 <= V <= 2^28, 0 <= E, F <= 2^28; sizes outside are MR_EINVAL (the workspace query returns
 * 0).  An index outside [0, V) in nbr or flaps skips that neighbour or flap.  Gather form, eight lanes per vertex,
 * no atomics and no zero-fills: each workgroup sums its part into one workspace row (forward only; needed unless
 * terms is 0) and a second launch adds an image's rows in a fixed order, so the results are bit-reproducible in
 * either deterministic mode and an image's terms do not depend on the rest of the batch. */
#define MR_MESH_LAPLACIAN 1
#define MR_MESH_EDGE 2
#define MR_MESH_NORMAL 4
size_t mr_mesh_regularizer_workspace_bytes(int B, int V, int F);
int mr_mesh_regularizer_forward(const float *vertices, const int32_t *nbr_offsets, const int32_t *nbr,
                                const int32_t *flaps, int B, int V, int E, int F, int terms, int use_target,
                                float target_length, float *unit_dirs, float *out_terms, void *workspace,
                                size_t workspace_bytes, void *stream);
int mr_mesh_regularizer_backward(const float *dterms, const float *vertices, const float *unit_dirs,
                                 const int32_t *nbr_offsets, const int32_t *nbr, const int32_t *flaps,
                                 const int32_t *role_offsets, const int32_t *roles, int B, int V, int E, int F,
                                 int terms, int use_target, float target_length, float *dvertices, void *stream);

/* ---- nearest neighbours between point clouds: the Chamfer distance (no reference counterpart) ----
 * Per image b, for every query x_i with i < x_lengths[b], over the targets y_j with j < y_lengths[b]
 * ("Point-cloud losses"):
 *   sqdist_i = min_j (x_i - y_j).(x_i - y_j)   in this difference form, never |x|^2 + |y|^2 - 2 x.y
 *   idx_i    = the LOWEST j that attains it (equal float32 distances), whatever the launch shape
 * A padded query (i >= x_lengths[b]) and every query of an image without targets get sqdist 0, idx -1.  Every idx
 * written for a valid query with a non-empty target lies in [0, y_lengths[b]), also when coordinates are NaN or
 * infinite (a distance that is NaN never wins; a query whose distances are all NaN gets sqdist +inf).
 *   x [B,N,3], y [B,M,3] f32;  x_lengths, y_lengths [B] i32 (device) or NULL = all N / all M; clamped to [0, N] /
 *   [0, M] by the kernels
 *   sqdist [B,N] f32 out or NULL;  idx [B,N] i32 out
 *   total  [B] f32 or NULL: total[b] = (accumulate ? total[b] : 0) + weight * (mean of sqdist over image b's valid
 *          queries; 0 when either side is empty) -- a fixed-order sum of per-workgroup partials, so Chamfer's two
 *          directions are two calls, the second with accumulate = 1
 * mr_nearest_plan: the launch shape of these sizes, a pure host function (nothing touches a device): the target
 * range is cut into `splits` runs of whole `target_tile`s (one workgroup of `workgroup_size` threads per run and
 * `queries_per_lane` x `workgroup_size` queries; with splits > 1 each writes a 64-bit key (distance bits << 32) |
 * index per query into the workspace and a second pass takes the unsigned minimum: order-independent, no atomics).
 * The workspace holds those keys and the partial sums; it is needed by every call (>= 256 bytes).
 *
 * mr_nearest_backward: the gradient of  sum_i g_i sqdist_i  of the directions that ran, to both clouds in one call:
 *   direction x -> y (idx_xy [B,N] non-NULL): dx_i += 2 g_i (x_i - y_idx_i),  dy_j -= sum_{i: idx_i = j} 2 g_i (x_i - y_j)
 *   direction y -> x (idx_yx [B,M] non-NULL): the same with the clouds exchanged
 *   g_i = grad_points[b,i]  (per point, [B,N], x -> y alone), or with grad_images [B]:
 *         grad_images[b] * x_weight / valid queries of x  (x -> y),   grad_images[b] * y_weight / valid y  (y -> x)
 *   order_xy [B,N], offsets_xy [B,M+1] i32: the inverted index of idx_xy -- per image the queries i grouped by their
 *         idx_i in ascending j, each group in a FIXED order (a stable sort of idx with -1 last), group j at
 *         order_xy[b, offsets_xy[b,j] .. offsets_xy[b,j+1]); needed when dy is asked for.  order_yx [B,M],
 *         offsets_yx [B,N+1] likewise for dx.
 *   dx [B,N,3], dy [B,M,3] f32 out or NULL (not computed); each is written completely, padded rows 0
 * Exactly one of grad_points / grad_images.  Gather form over the inverted index, eight lanes per destination point
 * and a fixed butterfly: no atomics, no zero-fills, bit-reproducible in either deterministic mode.  An index outside
 * the other cloud in idx or order is skipped.
 * 1 <= B <= 65535, 1 <= N, M <= 2^28, B * N and B * M below 2^36; sizes outside are MR_EINVAL (queries return 0). */
int mr_nearest_plan(int B, int N, int M, int *splits, int *queries_per_lane, int *target_tile, int *workgroup_size);
size_t mr_nearest_workspace_bytes(int B, int N, int M);
int mr_nearest_forward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B, int N,
                       int M, float *sqdist, int32_t *idx, float *total, float weight, int accumulate, void *workspace,
                       size_t workspace_bytes, void *stream);
int mr_nearest_backward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B, int N,
                        int M, const int32_t *idx_xy, const int32_t *order_xy, const int32_t *offsets_xy,
                        const int32_t *idx_yx, const int32_t *order_yx, const int32_t *offsets_yx,
                        const float *grad_points, const float *grad_images, float x_weight, float y_weight, float *dx,
                        float *dy, void *stream);

/* ---- K nearest neighbours between point clouds (no reference counterpart) ----
 * Per image b, for every query x_i with i < x_lengths[b], the K targets y_j with j < y_lengths[b] that have the K
 * SMALLEST 64-bit keys  (bits of (x_i - y_j).(x_i - y_j) << 32) | j,  in ascending key order (INTEGRATION.md,
 * "K nearest neighbours"); the distance in the difference form, as mr_nearest_forward.  Equal float32 distances go
 * to the lowest index, and a NaN distance (a bit pattern above +inf's) sorts after every number, whatever the launch
 * shape, the split count or K: the first K' columns of a K-neighbour call are the K'-neighbour call, bit for bit.
 *   x [B,N,3], y [B,M,3] f32;  x_lengths, y_lengths [B] i32 (device) or NULL, clamped to [0, N] / [0, M] by the kernels
 *   sqdist [B,N,K] f32 out, idx [B,N,K] i32 out.  A slot whose distance is NaN reports sqdist +inf; its idx, like
 *   every idx of a valid slot, lies in [0, y_lengths[b]).  A slot k >= y_lengths[b] and every slot of a padded query
 *   (i >= x_lengths[b]) get sqdist 0, idx -1.  Padded coordinates influence nothing.
 * mr_knn_plan: the launch shape, a pure host function: every lane keeps `queries_per_lane` sorted lists of
 * `list_capacity` keys (K rounded up to 4, 8, 16 or 32) in registers; the targets are cut into `splits` runs of whole
 * `target_tile`s as for mr_nearest_forward.  With splits > 1 every run writes its K keys per query into the workspace
 * (B * splits * N * K * 8 bytes, rounded up to 256; 0 without a split) and a second pass keeps the K smallest:
 * order-independent, no atomics.
 *
 * mr_knn_backward: the gradient of  sum_ik g_ik sqdist_ik  (grad [B,N,K] f32) from the saved sqdist and idx:
 *   dx_i = sum_k 2 g_ik (x_i - y_idx_ik),   dy_j = -sum_{(i,k): idx_ik = j} 2 g_ik (x_i - y_j)
 *   order [B,N*K], offsets [B,M+1] i32: the inverted index of idx flattened to [B,N*K] (entry e belongs to query
 *         e / K), as for mr_nearest_backward: a stable sort with -1 last; needed when dy is asked for
 *   dx [B,N,3], dy [B,M,3] f32 out or NULL (not computed); each is written completely, padded rows 0
 * A slot with idx -1, an idx outside the other cloud, or a sqdist that is not finite contributes nothing.  Eight
 * lanes per destination row and a fixed butterfly: no atomics, no zero-fills, bit-reproducible in either
 * deterministic mode.  All entry points only enqueue on `stream`: capturable in a HIP graph.
 * 1 <= K <= 32; B, N, M as for mr_nearest_forward, and N * K < 2^31, B * N * K < 2^36; anything else is MR_EINVAL
 * (queries return 0) before a device is touched. */
int mr_knn_plan(int B, int N, int M, int K, int *splits, int *queries_per_lane, int *list_capacity, int *target_tile,
                int *workgroup_size);
size_t mr_knn_workspace_bytes(int B, int N, int M, int K);
int mr_knn_forward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B, int N,
                   int M, int K, float *sqdist, int32_t *idx, void *workspace, size_t workspace_bytes, void *stream);
int mr_knn_backward(const float *x, const float *y, const int32_t *x_lengths, const int32_t *y_lengths, int B, int N,
                    int M, int K, const float *sqdist, const int32_t *idx, const int32_t *order, const int32_t *offsets,
                    const float *grad, float *dx, float *dy, void *stream);

/* ---- farthest-point sampling of point clouds (no reference counterpart) ----
 * Per cloud b with length_b = lengths[b] (N without lengths), K indices chosen greedily (INTEGRATION.md,
 * "Farthest-point sampling").  The definition is part of the interface:
 *   idx[b,0] = start_idx[b] clamped to [0, length_b) (0 without start_idx);
 *   every valid point carries a float32 running distance m_i: +inf, or 0 for a point with a non-finite coordinate,
 *   which is never updated;
 *   after the selection of s:  d_i = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)),  dx = fl(x_i - x_s), in un-fused
 *   binary32 in exactly this order;  m_i <- d_i if d_i < m_i (a NaN d_i changes nothing);  m_s <- -1;
 *   the next selection is the point with the largest m_i, the lowest index among equals.
 * The indices of a cloud are pairwise distinct whenever K <= length_b (a duplicate of a selected point has m = 0 > -1).
 *   points [B,N,3] f32;  lengths, start_idx [B] i32 (device) or NULL, clamped by the kernels
 *   idx [B,K] i32 out;  radius [B,K] f32 out: m of the selected point at the moment of its selection, +inf in slot 0,
 *   non-increasing from slot 1.  Slots k >= length_b get idx -1, radius 0.  Padded coordinates influence nothing.
 * Two routes with bit-identical results.  Route 1: one launch, one workgroup of `workgroup_size` lanes per cloud that
 * keeps `points_per_lane` points a lane in registers for all K steps (N <= 24576).  Route 2: one launch per step over
 * `slices` workgroups per cloud, the running distances in the workspace, K + 1 launches; stream order is the only
 * synchronisation between workgroups.  mr_farthest_plan: the route and launch shape the library takes (route 0 of
 * mr_farthest_forward), a pure host function; it depends on N alone.  route 1 / 2 force one; a forced route 1 whose
 * N it cannot hold is MR_EINVAL.  The workspace (B * N * 4 bytes rounded up to 256, plus 2 * B * slices * 32 for the
 * partial results; needed by every call) serves either route.  All entry points only enqueue on `stream`: capturable
 * in a HIP graph, nothing is read back.
 * 1 <= B <= 65535, 1 <= N < 2^28, 1 <= K < 2^24, B * K < 2^31; anything else is MR_EINVAL (queries return 0) before a
 * device is touched. */
int mr_farthest_plan(int B, int N, int K, int *route, int *workgroup_size, int *points_per_lane, int *slices);
size_t mr_farthest_workspace_bytes(int B, int N, int K);
int mr_farthest_forward(const float *points, const int32_t *lengths, const int32_t *start_idx, int B, int N, int K,
                        int route, int32_t *idx, float *radius, void *workspace, size_t workspace_bytes, void *stream);

/* ---- (I + lam L) over a mesh's adjacency: apply and conjugate-gradient solve (no reference counterpart) ----
 * A = I + lam L with L = D - Adj the combinatorial graph Laplacian of a symmetric CSR adjacency (nbr_offsets [V+1],
 * nbr [nnz] i32, as mesh_topology() builds it; INTEGRATION.md, "Preconditioned optimisation"):
 *   (A x)_i = (1 + lam deg_i) x_i - lam sum_{j in nbr(i)} x_j;   a vertex without neighbours has the identity row.
 * A is symmetric positive definite with smallest eigenvalue 1.  x, y, b, x0 are [B,V,C] f32 with 1 <= C <= 4, one
 * adjacency for the batch; every (image, channel) pair is a system of its own.  Offsets are clamped into [0, nnz] and
 * a neighbour outside [0, V) adds nothing, whatever the arrays hold.
 * mr_laplacian_apply: y = A x, one launch; the row is evaluated in float64 -- the neighbours summed in CSR order,
 * then (1 + lam deg_i) x_i - lam sum -- and rounded to float32 once.  The solve's q = A p is the same evaluation.
 * mr_laplacian_solve: x with A x = b by Jacobi-preconditioned conjugate gradients.  The algorithm is part of the
 * interface.  M = diag(1 + lam deg);  x = x0 (NULL: 0), r = b - A x, z = r / M, p = z, rho = r.z;  per iteration
 *   q = A p;  alpha = rho / p.q;  x += alpha p;  r -= alpha q;  z = r / M;  rho' = r.z;  p = z + (rho' / rho) p.
 * The vectors are float32; the dot products, alpha, beta and every row of A p are float64, rounded once where they meet
 * the vectors.
 * A system FREEZES the first time one of these holds, after which its x, iterations and residual never change again,
 * bit for bit, whatever the other systems of the call do:
 *   1. r.r <= tol^2 b.b, tested before the first iteration and after every one (b = 0 without x0: x = 0, 0 iterations);
 *   2. b.b or the initial r.r is not finite: the system's x is all NaN, 0 iterations, residual NaN;
 *   3. p.q <= 0 or not finite (breakdown): the system keeps the x it had before that iteration.
 *   iterations [B,C] i32 out: iterations performed;  residual [B,C] f32 out: sqrt(r.r / b.b) of the recurrence when
 *   the system froze or the iterations ran out, 0 for b = 0.
 * The order of every sum depends on (V, C, route) alone: a batch equals its single calls and a run with more
 * iterations equals the shorter one wherever that had frozen, bit for bit.  Two routes.  Route 1: one launch, one
 * workgroup of `workgroup_size` lanes per image holding `vertices_per_lane` vertices a lane in registers, p published
 * through LDS (V <= 3072).  Route 2: `slices` workgroups per image; one launch before the first iteration, two per
 * iteration and one at the end, partial dot products in the workspace summed by every workgroup of the next launch;
 * stream order is the only synchronisation between workgroups.  mr_laplacian_solve_plan: the route and launch shape
 * for `route` (0: the library's choice, a function of V and C alone; 1 / 2 forced; a forced route 1 that cannot hold
 * V is MR_EINVAL), a pure host function.
 * A call runs the iterations [first_iteration, first_iteration + iteration_count) cut at max_iterations: with
 * first_iteration = 0 it starts the solve, and when the range reaches max_iterations it ends it (iterations,
 * residual and rule 2's NaN are written then).  A range that stops short writes all_frozen [B] i32 (when given):
 * whether every system of image b is frozen, for a caller that reads it back to stop early -- by calling once more
 * with first_iteration = max_iterations.  Route 1 runs every iteration in the call with first_iteration = 0 and does
 * nothing in any other.  (0, max_iterations, NULL) is the whole solve, nothing read back.  The workspace (five
 * [B,V,C] f32 planes, the partials and the systems' state; needed by every call, it carries the solve between the
 * calls of one solve) serves either route.  All entry points only enqueue on `stream`: capturable in a HIP graph.
 * 1 <= B <= 65535, 1 <= V < 2^28, B V C < 2^36, nnz >= 0, lam >= 0 and finite, tol >= 0 and finite,
 * 0 <= max_iterations <= 10000, 0 <= first_iteration <= max_iterations; anything else is MR_EINVAL (the workspace
 * query returns 0) before a device is touched. */
int mr_laplacian_apply(const float *x, const int32_t *nbr_offsets, const int32_t *nbr, int B, int V, int C, int nnz,
                       float lam, float *y, void *stream);
int mr_laplacian_solve_plan(int V, int C, int route, int *chosen_route, int *workgroup_size, int *vertices_per_lane,
                            int *slices);
size_t mr_laplacian_solve_workspace_bytes(int B, int V, int C);
int mr_laplacian_solve(const float *b, const float *x0, const int32_t *nbr_offsets, const int32_t *nbr, int B, int V,
                       int C, int nnz, float lam, double tol, int max_iterations, int route, int first_iteration,
                       int iteration_count, int32_t *all_frozen, float *x, int32_t *iterations, float *residual,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ---- registration of matched point sets and the per-round chain of ICP (no reference counterpart) ----
 * Row-vector convention  s x R + T ~ y  ("Registration").  Per image b, over the KEPT rows i <
 * lengths[b] (N without lengths) with weight w_i (1 without weights) and match y_i, the definition is part of the
 * interface:
 *   W = sum w;  xm, ym the weighted means;  C = sum w (x - xm)(y - ym)^T / W = U S V^T;
 *   E = diag(1, 1, det(U V^T)), or I with allow_reflection;  R = U E V^T;
 *   s = tr(S E) / (sum w |x - xm|^2 / W) with estimate_scale and a positive denominator, else 1;  T = ym - s xm R;
 *   rmse = sqrt(max(0, s^2 var(x) - 2 s tr(S E) + var(y))), the weighted residual of (R, T, s) in closed form.
 * W = 0 gives R = I, T = 0, s = 1, rmse = 0.  C = 0 gives R = I; a rank-deficient C gives a finite orthonormal R of
 * the required determinant that attains the minimum residual (which one of several is not specified).  A non-finite
 * coordinate or weight in a kept row makes R, T, s and rmse of THAT image NaN.
 *   x [B,N,3] f32.  gather = 0: y [B,N,3] is matched row by row (M must equal N); idx [B,N] i32 or NULL then only
 *   marks rows, idx < 0 = dropped.  gather = 1: y [B,M,3] is read at idx [B,N] (required); idx outside [0, M) = dropped,
 *   and no gathered cloud is ever formed.  weights [B,N] f32 or NULL;  sqdist [B,N] f32 or NULL: a row is kept only
 *   while sqdist <= max_sqdist;  lengths [B] i32 or NULL, clamped by the kernels; padded rows influence nothing.
 *   R [B,3,3], T [B,3], s [B] f32 out;  rmse [B] f32 out or NULL.
 * Two launches: eighteen float64 moments summed per workgroup over fixed chunks of 1024 rows, each chunk about a
 * reference point of its own -- its first kept row of positive weight and that row's match, never a row that is not
 * counted -- and left in the workspace (B * ceil(N / 1024) * 144 bytes rounded up to 256) as the chunk's W, means and
 * moments centred on those means; the chunks are merged in a fixed order, no atomics -- the result of an image does not
 * depend on the padding or the other images of its batch, nor on the coordinates of a row with weight 0 (finite ones)
 * or of a dropped or padded row (any); then one lane per image in float64: a cyclic one-sided Jacobi SVD with a fixed
 * sweep bound, rounded to float32 once at the end.
 * ICP's bookkeeping, all three given or all NULL (rmse is then required): converged [B] i32, iterations [B] i32,
 * prev_rmse [B] f64 (8-byte aligned), initialised by mr_align_icp_init.  An image with converged != 0 is left untouched,
 * bit for bit.  Otherwise iterations += 1 and, with the float64 rmse before rounding: converged = 1 when rmse == 0 or,
 * from the image's second round on, (prev_rmse - rmse) / prev_rmse <= relative_rmse_thr; prev_rmse = rmse.  W = 0
 * then means "no kept match": converged = 1, rmse = 0, and R, T, s keep their values.
 * mr_align_apply: xt [B,N,3] = s x R + T in float32, 0 in padded rows.  mr_align_closest_points: out [B,N,3] = the sum
 * of bary * corner for mr_nearest_triangle_forward's (face [B,N], bary [B,N,3]), 0 where face is -1 or names a
 * triangle with an index outside [0, V).  mr_align_icp_init: R0 / T0 / s0 (all given or all NULL: the identity) into
 * R, T, s; rmse 0, converged 0, iterations 0.  All entry points only enqueue on `stream`: capturable in a HIP graph,
 * nothing is read back.
 * B, N, M, V, T as mr_nearest_forward / mr_nearest_triangle_forward take them (1 <= B <= 65535, 1..2^28 rows, B * rows
 * < 2^36); anything else is MR_EINVAL (the query returns 0) before a device is touched. */
size_t mr_align_workspace_bytes(int B, int N);
int mr_align_solve(const float *x, const float *y, const int32_t *idx, int gather, const float *weights,
                   const float *sqdist, float max_sqdist, const int32_t *lengths, int B, int N, int M,
                   int estimate_scale, int allow_reflection, double relative_rmse_thr, float *R, float *T, float *s,
                   float *rmse, int32_t *converged, int32_t *iterations, double *prev_rmse, void *workspace,
                   size_t workspace_bytes, void *stream);
int mr_align_apply(const float *x, const int32_t *lengths, const float *R, const float *T, const float *s, int B, int N,
                   float *xt, void *stream);
int mr_align_closest_points(const float *vertices, const int32_t *triangles, const int32_t *face, const float *bary,
                            int B, int N, int V, int T, float *out, void *stream);
int mr_align_icp_init(const float *R0, const float *T0, const float *s0, int B, float *R, float *T, float *s,
                      float *rmse, int32_t *converged, int32_t *iterations, double *prev_rmse, void *stream);

/* ---- point to nearest triangle: the point-to-mesh distance (no reference counterpart) ----
 * Per image b, for every query p_i with i < lengths[b], over the T triangles of one shared topology
 * ("Point-cloud losses"):
 *   sqdist_i = min_t dist^2(p_i, triangle t)   to the CLOSED triangle: interior, edges and corners
 *   face_i   = the LOWEST t that attains it (equal float32 distances), whatever the launch shape
 *   bary_i   = the barycentrics of the closest point c_i = sum_k bary_ik v_k on that triangle, >= 0
 * dist^2(p, (a, b, c)) with e0 = b - a, e1 = c - a, d = p - a is the least of: the plane projection when
 * det = |e0|^2 |e1|^2 - (e0.e1)^2 > 0 and its coordinates satisfy v >= 0, w >= 0, v + w <= 1, and the closest points
 * of the segments ab, bc, ca (parameter clamped to [0, 1]; a zero-length segment is its end point) -- each evaluated
 * as |d - (beta e0 + gamma e1)|^2, never from an absolute closest point.  A zero-area triangle is its edges or its
 * point: a finite distance.  A triangle with an index outside [0, V) is never chosen.  A padded query, and a query
 * for which no triangle compared below +inf (no usable triangle, NaN coordinates), get sqdist 0, face -1, bary 0;
 * every other face written is a usable triangle's index.
 *   points [B,N,3], vertices [B,V,3] f32;  triangles [T,3] i32;  lengths [B] i32 (device) or NULL = all N
 *   sqdist [B,N] f32 out or NULL;  face [B,N] i32 out;  bary [B,N,3] f32 out
 *   total  [B] f32 out or NULL: the mean of sqdist over image b's valid queries (0 without one), a fixed-order sum
 * mr_nearest_triangle_plan: the launch shape, a pure host function: the triangles are cut into `splits` runs of
 * whole `triangle_tile`s, a workgroup of `workgroup_size` threads holds `queries_per_lane` x `workgroup_size` queries;
 * with splits > 1 the runs meet through 64-bit keys as in mr_nearest_forward.  The workspace holds the per-image
 * triangle records (80 bytes each), those keys and the partial sums; 16-byte aligned, needed by every call.
 *
 * mr_nearest_triangle_backward: the gradient of  sum_i g_i sqdist_i  with the barycentrics held constant (the
 * envelope theorem):  dpoints_i = 2 g_i (p_i - c_i),  dvertices_k -= 2 g_i bary_ik (p_i - c_i)  for the corners k of
 * face_i;  g_i = grad_points[b,i] ([B,N]) or grad_images[b] / valid queries ([B], the mean's upstream): exactly one.
 *   order [B,3N], offsets [B,V+1] i32: the inverted index of the entries 3 i + k keyed by the vertex
 *         triangles[face_i][k] (-1 for rows without a face), each vertex's entries in a FIXED order (a stable sort,
 *         as for mr_nearest_backward); needed when dvertices is asked for
 *   dpoints [B,N,3], dvertices [B,V,3] f32 out or NULL (not computed); each is written completely
 * No atomics, no zero-fills, bit-reproducible in either deterministic mode.
 * 1 <= B <= 65535, 1 <= N, V, T <= 2^28, B * N, B * V and B * T below 2^36; sizes outside are MR_EINVAL (queries
 * return 0). */
int mr_nearest_triangle_plan(int B, int N, int T, int *splits, int *queries_per_lane, int *triangle_tile,
                             int *workgroup_size);
size_t mr_nearest_triangle_workspace_bytes(int B, int N, int T);
int mr_nearest_triangle_forward(const float *points, const float *vertices, const int32_t *triangles,
                                const int32_t *lengths, int B, int N, int V, int T, float *sqdist, int32_t *face,
                                float *bary, float *total, void *workspace, size_t workspace_bytes, void *stream);
int mr_nearest_triangle_backward(const float *points, const float *vertices, const int32_t *triangles,
                                 const int32_t *lengths, int B, int N, int V, int T, const int32_t *face,
                                 const float *bary, const int32_t *order, const int32_t *offsets,
                                 const float *grad_points, const float *grad_images, float *dpoints, float *dvertices,
                                 void *stream);

/* ---- triangle to nearest point: the mesh-to-point distance (no reference counterpart) ----
 * The other direction of the search above, with the same pair arithmetic: dist^2(p, t) of a (point, triangle) pair is
 * the same float32 number in both.  Per image b, for every triangle t of the shared topology, over the points p_j
 * with j < lengths[b] ("Point-cloud losses"):
 *   sqdist_t = min_j dist^2(p_j, triangle t)   from the CLOSED triangle, dist^2 as defined above
 *   index_t  = the LOWEST j that attains it (equal float32 distances), whatever the launch shape
 *   bary_t   = the barycentrics of the triangle's closest point c_t to p_index_t, >= 0
 * A triangle with an index outside [0, V), and a triangle for which no point compared below +inf (lengths[b] = 0,
 * NaN coordinates, a point at +-inf), get sqdist 0, index -1, bary 0; every other index lies in [0, lengths[b]).
 *   points [B,N,3], vertices [B,V,3] f32;  triangles [T,3] i32;  lengths [B] i32 (device) or NULL = all N
 *   sqdist [B,T] f32 out or NULL;  index [B,T] i32 out;  bary [B,T,3] f32 out
 *   usable [B] i32 out or NULL: U, the triangles with every index in [0, V) (the same for every image), counted on
 *          the device; needed with total, and by the backward of the mean
 *   total  [B] f32 out or NULL: the sum of sqdist over image b's triangles / U in a fixed order (a usable triangle
 *          without a result adds 0 and counts); 0 when U = 0 or the image has no valid point
 * mr_nearest_point_of_triangle_plan: the launch shape, a pure host function: one triangle a lane, `workgroup_size`
 * triangles a workgroup; the cloud is cut into `splits` runs of whole `point_tile`s, which meet through 64-bit keys
 * (distance bits << 32) | point index as in mr_nearest_forward; `points_per_step` is 2 where the points are visited
 * as packed fp32 pairs.  The workspace holds the per-image triangle records (80 bytes each), those keys and the
 * partial sums; 16-byte aligned, needed by every call.
 *
 * mr_nearest_point_of_triangle_backward: the gradient of  sum_t g_t sqdist_t  with the barycentrics held constant:
 *   dvertices_k = -sum 2 g_t bary_tk (p_index_t - c_t)  over the corners that name vertex k,
 *   dpoints_j   =  sum_{t: index_t = j} 2 g_t (p_j - c_t);
 *   g_t = grad_triangles[b,t] ([B,T]) or grad_images[b] / usable[b] ([B], the mean's upstream): exactly one.
 *   corner_order [B,3T], corner_offsets [B,V+1] i32: the inverted index of the entries 3 t + k keyed by the vertex
 *         triangles[t][k] (-1 for triangles without a result); needed when dvertices is asked for
 *   point_order [B,T], point_offsets [B,N+1] i32: the inverted index of index (triangles grouped by the point they
 *         chose); needed when dpoints is asked for.  Both as for mr_nearest_backward: a stable sort, -1 last.
 *   dpoints [B,N,3], dvertices [B,V,3] f32 out or NULL (not computed); each is written completely, rows that nobody
 *         names 0
 * No atomics, no zero-fills, bit-reproducible in either deterministic mode.  Limits as for mr_nearest_triangle_*. */
int mr_nearest_point_of_triangle_plan(int B, int N, int T, int *splits, int *points_per_step, int *point_tile,
                                      int *workgroup_size);
size_t mr_nearest_point_of_triangle_workspace_bytes(int B, int N, int T);
int mr_nearest_point_of_triangle_forward(const float *points, const float *vertices, const int32_t *triangles,
                                         const int32_t *lengths, int B, int N, int V, int T, float *sqdist,
                                         int32_t *index, float *bary, float *total, int32_t *usable, void *workspace,
                                         size_t workspace_bytes, void *stream);
int mr_nearest_point_of_triangle_backward(const float *points, const float *vertices, const int32_t *triangles,
                                          const int32_t *lengths, int B, int N, int V, int T, const int32_t *index,
                                          const float *bary, const int32_t *corner_order,
                                          const int32_t *corner_offsets, const int32_t *point_order,
                                          const int32_t *point_offsets, const float *grad_triangles,
                                          const float *grad_images, const int32_t *usable, float *dpoints,
                                          float *dvertices, void *stream);

/* ---- winding number: on which side of the mesh a point lies (no reference counterpart) ----
 * The generalized winding number (Jacobson et al. 2013) of one shared topology around every query: per image b, for
 * p = points[b,i] with i < lengths[b], over the triangles f with corners va, vb, vc = vertices[b, triangles[f]]
 * ("Point-cloud losses"), in float32:
 *   a = va - p, b = vb - p, c = vc - p
 *   num = a . (b x c),   den = |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|
 *   t_f = 2 atan2(num, den) / (4 pi)   (|t_f| <= 0.5, atan2(0, 0) = 0),     w[b,i] = sum_f t_f
 * 1 inside and 0 outside a closed mesh whose triangles are counter-clockwise seen from outside; in between for an
 * open or folded one.  A triangle with an index outside [0, V) or with two equal indices is skipped; a geometrically
 * degenerate triangle with three distinct indices is evaluated like any other.
 * The sum is ORDER-FREE: every t_f is rounded to the nearest multiple of 2^-40 (ties to even), the rounded terms are
 * added exactly in 64-bit integers and w = (float)(sum 2^-40), rounded once -- the same bits whatever the order of
 * the triangles, the launch shape or the batch the image sat in (csrc/wn_fixed.h).  T > 2^24 is MR_EINVAL: the sum
 * could leave the 64-bit range.  A padded query gets 0.  A query that met a num or a den that is not finite (a NaN or
 * infinite point, a NaN vertex of a usable triangle, coordinates whose products overflow) gets NaN; other queries
 * and other images are unaffected.  There is no backward: w is piecewise constant for a closed mesh.
 *   points [B,N,3], vertices [B,V,3] f32;  triangles [T,3] i32;  lengths [B] i32 (device) or NULL = all N
 *   w [B,N] f32 out
 * mr_winding_number_plan: the launch shape, a pure host function, as mr_nearest_triangle_plan; with splits > 1 the
 * runs of triangles meet through one 64-bit integer partial per (image, split, query), written with plain stores and
 * added by a second launch: no atomics, stream order only, capturable.  The workspace holds the per-image triangle
 * records (48 bytes each) and those partials; 16-byte aligned, needed by every call.
 * 1 <= B <= 65535, 1 <= N, V <= 2^28, 1 <= T <= 2^24, B * N, B * V and B * T below 2^36; sizes outside are
 * MR_EINVAL (queries return 0). */
int mr_winding_number_plan(int B, int N, int T, int *splits, int *queries_per_lane, int *triangle_tile,
                           int *workgroup_size);
size_t mr_winding_number_workspace_bytes(int B, int N, int T);
int mr_winding_number_forward(const float *points, const float *vertices, const int32_t *triangles,
                              const int32_t *lengths, int B, int N, int V, int T, float *w, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ---- ray casting: where a ray first meets the mesh (no reference counterpart) ----
 * Per image b, for every ray (o, d) = (origins[b,i], directions[b,i]) with i < lengths[b], over the triangles f of one
 * shared topology with corners va, vb, vc = vertices[b, triangles[f]]: the watertight test of Woop, Benthin and Wald
 * (2013), in float32 ("Point-cloud losses").  d is NOT normalised: t is in units of |d|, the hit point
 * is o + t d.
 *   per ray:     kz = the first of x, y, z that attains max |d_k|;  kx = (kz + 1) % 3, ky = (kz + 2) % 3, exchanged
 *                when d[kz] < 0;  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]
 *   per corner:  p = v_P - o;  Px = fma(-Sx, p[kz], p[kx]),  Py = fma(-Sy, p[kz], p[ky]),  Pz = Sz p[kz]
 *   edges:       U = Cx By - Cy Bx,  V = Ax Cy - Ay Cx,  W = Bx Ay - By Ax: two rounded products and one rounded
 *                difference each, never fused, so the neighbour across a shared edge computes the exact negative.
 *                If any of the three is exactly 0, all three are recomputed in float64 from the float32 Ax .. Cy (the
 *                products are exact there, so the signs are), the sign test below is made on the float64 values, and
 *                they are rounded to float32 for what follows.
 *   acceptance:  every step is a comparison that a NaN fails.  Reject when some edge function is < 0 and some is > 0;
 *                det = (U + V) + W, reject when det == 0;  T = (U Az + V Bz) + W Cz (each operation rounded),
 *                t = T / det rounded once; accept when t >= t_min && t <= t_max; -0 is stored as +0.
 *                bary = (U, V, W) / det.
 * The first hit is the accepted triangle with the least t; equal t goes to the lowest face; a t of +inf is no hit.
 * A triangle with an index outside [0, V), two equal indices or a corner that is not finite is never hit.  A ray
 * without a hit -- a padded row, a non-finite origin or direction, a zero direction, nothing in [t_min, t_max] --
 * gets t = +inf, face = -1, bary = 0.  No back-face culling.  0 <= t_min <= t_max, else MR_EINVAL.
 * A ray's t, face and bary are the same bit for bit whatever the launch shape or the batch the image sat in: a finish
 * pass evaluates the chosen pair once more with the search's own functions.
 *   origins, directions [B,N,3], vertices [B,V,3] f32;  triangles [T,3] i32;  lengths [B] i32 (device) or NULL = all N
 *   t [B,N] f32, face [B,N] i32, bary [B,N,3] f32 out
 * mr_cast_rays_plan: the launch shape, a pure host function, as mr_winding_number_plan; with splits > 1 the runs of
 * triangles meet through one 64-bit (t bits, face) key per (image, split, ray), written with plain stores and merged
 * by a second launch: no atomics, stream order only, capturable.  The workspace holds the per-image corner records (48
 * bytes each) and those keys; 16-byte aligned, needed by every forward call.
 * Backward, the face held fixed: with n = (vb - va) x (vc - va) and g = n / (n . d)
 *   dorigins[b,i] = -grad_t[b,i] g,  ddirections[b,i] = -grad_t[b,i] t[b,i] g,
 *   dvertices[b,v] = sum over the (ray, corner k) that name v of grad_t[b,i] bary[b,i,k] g
 * 0, never NaN, for a ray without a hit, with n . d == 0 or with a g that is not finite.  Any of the three outputs may
 * be NULL (not computed).  dvertices is a gather over order [B,3N] / offsets [B,V+1], the inverted index of the
 * (ray, corner) entries keyed by vertex as mr_nearest_triangle_backward takes it; bitwise reproducible.
 * Size limits: those of mr_winding_number_*; sizes outside are MR_EINVAL (queries return 0). */
int mr_cast_rays_plan(int B, int N, int T, int *splits, int *queries_per_lane, int *triangle_tile,
                      int *workgroup_size);
size_t mr_cast_rays_workspace_bytes(int B, int N, int T);
int mr_cast_rays_forward(const float *origins, const float *directions, const float *vertices,
                         const int32_t *triangles, const int32_t *lengths, int B, int N, int V, int T, float t_min,
                         float t_max, float *t, int32_t *face, float *bary, void *workspace, size_t workspace_bytes,
                         void *stream);
int mr_cast_rays_backward(const float *directions, const float *vertices, const int32_t *triangles,
                          const int32_t *lengths, int B, int N, int V, int T, const float *t, const int32_t *face,
                          const float *bary, const int32_t *order, const int32_t *offsets, const float *grad_t,
                          float *dorigins, float *ddirections, float *dvertices, void *stream);

/* ---- clip-space transforms --------------------------------------------------------------
 * perspective(aspect, fov_y, near, far) . look_at(eye, center, up) per image, the product render() and
 * rasterize() apply to the vertices (src/common/camera_utils.py:45-139; src/mesh_renderer/render.py
 * :187-193), as one launch on cameras that live on the device, and its backward to eye / center / up
 * (one launch; fov_y, near, far are not differentiated).
 *   eye, center, up [B,3] f32; fov_y (degrees), near_clip, far_clip [B] f32; aspect = width / height
 *   transforms [B,4,4] f32 out, row-major
 *   degenerate  1 int32 out (device): bit 0 = some |center - eye| <= 1e-6, bit 1 = some
 *               |forward x up| <= 1e-6 on a camera that has a forward vector (bit 0 not raised by
 *               it) -- the two conditions the reference asserts on, in its order
 *               (camera_utils.py:68-69, 74-76); a NaN input raises both; the caller decides when
 *               to read it back
 *   dtransforms [B,4,4] f32; deye, dcenter, dup [B,3] f32 out */
int mr_camera_transforms(const float *eye, const float *center, const float *up, const float *fov_y,
                         const float *near_clip, const float *far_clip, float aspect, int B, float *transforms,
                         int32_t *degenerate, void *stream);
int mr_camera_transforms_backward(const float *dtransforms, const float *eye, const float *center,
                                  const float *up, const float *fov_y, const float *near_clip,
                                  const float *far_clip, float aspect, int B, float *deye, float *dcenter,
                                  float *dup, void *stream);

/* ---- tone_mapper ------------------------------------------------------------------------
 * Replaces tone_mapper (src/mesh_renderer/render.py:389-419): per image,
 *   out = clamp(image^gamma / max(image^gamma), 0, 1)     (torch.pow / torch.max / torch.clamp
 * semantics, NaNs included).  image: B images of `elements_per_image` floats each; max_scratch: B
 * ints (device, overwritten: the per-image maxima as float bits); exactly one of out_f32 (same
 * shape as image) and out_u8 (8-bit frames, the examples' `(x * 255).astype(np.uint8)` applied to
 * the tone-mapped value) is non-NULL. */
int mr_tone_map(const float *image, int B, size_t elements_per_image, float gamma, int32_t *max_scratch,
                float *out_f32, uint8_t *out_u8, void *stream);

/* ---- deterministic mode ------------------------------------------------------------------
 * The reference accumulates its gradients sequentially (rasterize_triangles.cpp:156-157, 232-269) and
 * is bit-reproducible; the default kernels here end in float atomics, whose sums depend on the order
 * in which wavefronts commit (last-bit differences from run to run).  mr_set_deterministic(1) makes
 * the calling thread's later mr_shade_backward / mr_shade_backward_l1 / mr_rasterize_backward calls
 * accumulate in 64-bit FIXED POINT with integer atomics instead -- integer addition is associative,
 * so the result is independent of that order -- followed by fixed-order per-vertex gathers.  The
 * fixed-point scale is a power of two derived on the device from the largest upstream gradient g:
 * contributions below g * 2^-42 are rounded away, a per-triangle total may reach g * 2^21.  About
 * 10 % slower (8-byte atomics, one extra pass to find g when the upstream is a dense image).
 * mr_shade_backward needs the vertex adjacency in this mode (MR_EINVAL without).  Round 3 extends the
 * mode to mr_interpolate_raster_backward and mr_shade_specular_backward (the latter needs the
 * adjacency too).  A contribution that does not fit the fixed-point range (NaN, infinite, beyond
 * 2^63 after scaling) raises a flag and the outputs of that call are NaN instead of a finite wrong
 * number.  mr_soft_backward is covered as well (fixed-point integer atomics into 64-bit copies of its
 * four vertex outputs, scaled for the 1 / sigma and 1 / gamma its contributions carry; its light
 * gradients are fixed-order sums in either mode).  mr_antialias_backward is covered (fixed-point integer atomics for dclip, scaled from a first pass that finds
 * its largest per-vertex contribution).  mr_sh_shade_backward has no atomics and is bit-reproducible in either mode, and so are mr_mesh_regularizer_forward / _backward, mr_ssim_forward / _backward and mr_nearest_forward / _backward.  mr_texture_backward is covered (fixed-point integer adds, in LDS and in the workspace, for dtex, scaled from a first pass that finds the largest upstream gradient and from the number of pixels that sample one texture; duv is per pixel in either mode), and so is mr_texture_mip_backward (the same fixed-point scatter into every level of the gradient pyramid, the same scale rule -- a contribution is level weight x tap weight x dout, at most |dout| -- then one gathered pass that converts each level's sums and folds them in a fixed order).  mr_texture_mip_forward and mr_attribute_derivatives have no atomics.  Not covered, float atomics remain: the composed
 * interpolation backward (mr_interpolate_backward, the path for more than 16 attributes).  mr_l1_loss_forward is always deterministic.  Returns the previous setting. */
int mr_set_deterministic(int on);

/* ---- kernel timing (measurement, no reference counterpart) ----------------------------
 * Arms ONE measurement: the next launch of the named kernel made BY THE CALLING THREAD records
 * hipEvent `start_event` immediately before and `stop_event` immediately after that kernel on
 * the call's stream, then the slot clears itself (one-shot, thread-local: a forgotten or a
 * concurrent caller's timer cannot attach to somebody else's launch).  bench.py's roofline legs
 * time single kernels inside a full step this way.  Results are unaffected.  NULL, NULL disarms. */
#define MR_TIMER_RASTER_FORWARD 0  /* k_raster: the forward G-buffer kernel of mr_rasterize_forward   */
#define MR_TIMER_SHADE_BACKWARD 1  /* the pixel pass of mr_shade_backward (fused shading backward)    */
#define MR_TIMER_SHADE_FORWARD 2   /* the pixel pass of mr_shade_forward                              */
#define MR_TIMER_RASTER_BACKWARD 3 /* the pixel pass of mr_rasterize_backward                         */
#define MR_TIMER_L1_FORWARD 4      /* the streaming pass of mr_l1_loss_forward                        */
#define MR_TIMER_COUNT 5
int mr_time_next_kernel(int which, void *start_event, void *stop_event);
/* The named kernel will NOT run in this step after all (mean|image - target| came out of mr_render_forward_l1): the
 * calling thread's armed pair, if any, is recorded on `stream` back to back -- an empty interval, so that a reader
 * of the pair finds two recorded events and a time of (nearly) zero instead of events that never happened, and the
 * pair does not wait for some later launch of that kernel -- and the slot clears. */
int mr_time_no_kernel(int which, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MESH_RASTER_H_ */
