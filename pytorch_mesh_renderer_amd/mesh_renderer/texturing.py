"""Differentiable texture mapping: bilinear, or mipmapped trilinear.

texture() samples an image-sized buffer of UV coordinates from a texture and is differentiable in both the texture
and the UVs; render_textured() rasterizes a mesh with per-corner UVs, samples its albedo from a texture and shades
it unlit or under second-order SH lighting.  texture_filtered() and render_textured_filtered() are the same two with
a choice of filter (filter_mode="linear-mipmap-linear": mipmapped trilinear); attribute_derivatives() gives the
screen-space UV derivatives that mode's level of detail needs.  The semantics are in INTEGRATION.md, "Texture
mapping"; the HIP kernels are csrc/texture.hip and csrc/texture_mip.hip.  render() and render_sh() are not touched:
textures come in through these entry points only.
"""
import torch

from .. import _native
from ..common import camera_utils
from .render import _per_batch, _per_batch_vec3
from .sh_lighting import SHShade, _sh_batch

_BOUNDARY_MODES = ("wrap", "clamp")
_FILTER_MODES = ("linear", "linear-mipmap-linear")


class TextureSample(torch.autograd.Function):
    """Bilinear sampling of tex at uv as one autograd op (one HIP pass each way); mask gets no gradient."""

    @staticmethod
    def forward(ctx, tex, uv, mask, boundary_mode):
        tex, uv = tex.detach(), uv.detach()
        mask = mask.detach() if mask is not None else None
        ctx.boundary_mode = boundary_mode
        ctx.save_for_backward(tex, uv, mask)
        return _native.texture_forward(tex, uv, mask, boundary_mode)

    @staticmethod
    def backward(ctx, dout):
        tex, uv, mask = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not (need[0] or need[1]):
            return None, None, None, None
        dtex, duv = _native.texture_backward(dout, tex, uv, mask, ctx.boundary_mode, want_tex=need[0],
                                             want_uv=need[1])
        return dtex, duv, None, None


class TextureMipSample(torch.autograd.Function):
    """Mipmapped trilinear sampling of tex at uv as one autograd op: the pyramid is built in the forward and saved
    for the backward.  uv_da and mask get no gradient: the level of detail is a filter-width decision, a constant."""

    @staticmethod
    def forward(ctx, tex, uv, uv_da, mask, boundary_mode, max_mip_level):
        tex, uv, uv_da = tex.detach(), uv.detach(), uv_da.detach()
        mask = mask.detach() if mask is not None else None
        ctx.boundary_mode, ctx.max_mip_level = boundary_mode, max_mip_level
        out, pyramid = _native.texture_mip_forward(tex, uv, uv_da, mask, boundary_mode, max_mip_level)
        ctx.save_for_backward(tex, pyramid, uv, uv_da, mask)
        return out

    @staticmethod
    def backward(ctx, dout):
        tex, pyramid, uv, uv_da, mask = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not (need[0] or need[1]):
            return None, None, None, None, None, None
        dtex, duv = _native.texture_mip_backward(dout, tex, pyramid, uv, uv_da, mask, ctx.boundary_mode,
                                                 ctx.max_mip_level, want_tex=need[0], want_uv=need[1])
        return dtex, duv, None, None, None, None


def _check_filter_args(filter_mode, max_mip_level):
    if filter_mode not in _FILTER_MODES:
        raise ValueError("filter_mode must be 'linear' or 'linear-mipmap-linear', got %r." % (filter_mode,))
    if max_mip_level is not None and (isinstance(max_mip_level, bool) or not isinstance(max_mip_level, int)
                                      or max_mip_level < 0):
        raise ValueError("max_mip_level must be None or a non-negative integer, got %r." % (max_mip_level,))


def texture_mip_levels(texture_height, texture_width, max_mip_level=None):
    """The number of pyramid levels "linear-mipmap-linear" uses for a texture of these extents:
    1 + min(tz(Ht), tz(Wt), max_mip_level), tz the number of trailing zero bits (a level exists while both extents
    of the one below are even)."""
    _check_filter_args("linear", max_mip_level)
    return _native.texture_mip_levels(texture_height, texture_width, max_mip_level)


def attribute_derivatives(ids, bary, clip_vertices, triangles, attributes, attribute_triangles=None):
    """Screen-space derivatives of perspective-correctly interpolated attributes; returns [B,H,W,A,2] float32.

    ids [B,H,W] int32 and bary [B,H,W,3]: the rasterizer's G-buffer for clip_vertices [B,V,4] and triangles [T,3]
    int32.  attributes [B,Va,A] or [Va,A] float32, 1 <= A <= 4, read corner by corner through attribute_triangles
    [T,3] int32 when given, else per vertex through `triangles` (Va = V).  out[..., a, 0] is the change of attribute
    a per step of one pixel column (X), out[..., a, 1] per step of one pixel row (Y) of the G-buffer, computed
    analytically from the rasterizer's edge functions; background pixels are 0.  Forward only: nothing here is
    differentiated.  For A = 2 (u, v) the result viewed as [B,H,W,4] is the `uv_da` of texture_filtered()."""
    if not torch.is_tensor(clip_vertices) or clip_vertices.dim() != 3 or clip_vertices.shape[2] != 4:
        raise ValueError("clip_vertices must have shape [batch_size, vertex_count, 4].")
    if not torch.is_tensor(attributes) or attributes.dim() not in (2, 3) or not 1 <= attributes.shape[-1] <= 4:
        raise ValueError("attributes must have shape [count, A] or [batch_size, count, A] with 1 <= A <= 4.")
    if attributes.dim() == 2:
        attributes = attributes.unsqueeze(0).expand(clip_vertices.shape[0], *attributes.shape)
    return _native.attribute_derivatives(ids.detach(), bary.detach(), clip_vertices.detach(), triangles,
                                         attributes.detach(), attribute_triangles)


def _check_texture_args(tex, uv, mask, boundary_mode):
    if not torch.is_tensor(uv) or uv.dim() != 4 or uv.shape[3] != 2:
        raise ValueError("uv must have shape [batch_size, height, width, 2].")
    batch_size, height, width = uv.shape[:3]
    if not torch.is_tensor(tex) or tex.dim() not in (3, 4) or (tex.dim() == 4 and tex.shape[0] != batch_size):
        raise ValueError("tex must have shape [Ht, Wt, C] or [batch_size, Ht, Wt, C].")
    if not 1 <= tex.shape[-1] <= 4:
        raise ValueError("tex must have 1 to 4 channels, got %d." % tex.shape[-1])
    if tex.shape[-3] < 1 or tex.shape[-2] < 1:
        raise ValueError("tex must have at least one texel.")
    if tex.dtype != torch.float32 or uv.dtype != torch.float32:
        raise ValueError("tex and uv must be float32.")
    if mask is not None and (not torch.is_tensor(mask) or list(mask.shape) != [batch_size, height, width]
                             or mask.dtype != torch.float32):
        raise ValueError("mask must be a float32 tensor of shape [batch_size, height, width] matching uv.")
    if boundary_mode not in _BOUNDARY_MODES:
        raise ValueError("boundary_mode must be 'wrap' or 'clamp', got %r." % (boundary_mode,))


def _check_corner_indices(uv_triangles, uv_count):
    """uv_triangles must index rows of uvs: the interpolation kernel reads them unchecked.  The check reads the
    range back to the host once per tensor and contents (cached on the tensor object, like antialias_topology);
    while a stream is being captured it cannot, and relies on the eager warm-up steps of capture_step."""
    key = (uv_triangles._version, int(uv_count), uv_triangles.data_ptr())
    if getattr(uv_triangles, "_mr_checked_uv_count", None) == key or uv_triangles.numel() == 0:
        return
    if uv_triangles.is_cuda and torch.cuda.is_current_stream_capturing():
        return
    lo, hi = int(uv_triangles.min()), int(uv_triangles.max())
    if lo < 0 or hi >= uv_count:
        raise ValueError("uv_triangles must index rows of uvs: got indices in [%d, %d] for %d rows." % (
            lo, hi, uv_count))
    try:
        uv_triangles._mr_checked_uv_count = key
    except AttributeError:
        pass


def texture(tex, uv, mask=None, boundary_mode="wrap"):
    """Bilinear texture lookup; returns [B,H,W,C] float32.

    tex [Ht,Wt,C] (shared by every image) or [B,Ht,Wt,C] float32 with 1 <= C <= 4; uv [B,H,W,2] float32;
    mask [B,H,W] float32 or None.  Coordinates follow grid_sample(align_corners=False): texel (i, j) =
    tex[..., i, j, :] covers u in [j/Wt, (j+1)/Wt) and v in [i/Ht, (i+1)/Ht), and row 0 of the tensor is v = 0
    (an image stored top row first, with v-up UVs, must be flipped by the caller).  boundary_mode "wrap" takes
    tap indices modulo the size, "clamp" clamps them to the edge.  A pixel is 0, and passes no gradient, where
    mask <= 0.5, where u or v is not finite, or where |u * Wt - 0.5| or |v * Ht - 0.5| >= 2^24.  Differentiable
    in tex (a shared texture's gradient sums over the batch) and uv.  texture_filtered() is the same lookup with a
    choice of filter (mipmapped trilinear).  Full statement: INTEGRATION.md, "Texture mapping"."""
    _check_texture_args(tex, uv, mask, boundary_mode)
    return TextureSample.apply(tex, uv, mask, boundary_mode)


def texture_filtered(tex, uv, mask=None, boundary_mode="wrap", uv_da=None, filter_mode="linear", max_mip_level=None):
    """Bilinear or mipmapped trilinear texture lookup; returns [B,H,W,C] float32.

    texture() with a choice of filter: its signature is pinned, so the filter arguments live here.  tex [Ht,Wt,C] (shared by every image) or [B,Ht,Wt,C] float32 with 1 <= C <= 4; uv [B,H,W,2] float32;
    mask [B,H,W] float32 or None.  Coordinates follow grid_sample(align_corners=False): texel (i, j) =
    tex[..., i, j, :] covers u in [j/Wt, (j+1)/Wt) and v in [i/Ht, (i+1)/Ht), and row 0 of the tensor is v = 0
    (an image stored top row first, with v-up UVs, must be flipped by the caller).  boundary_mode "wrap" takes
    tap indices modulo the size, "clamp" clamps them to the edge.  A pixel is 0, and passes no gradient, where
    mask <= 0.5, where u or v is not finite, or where |u * Wt - 0.5| or |v * Ht - 0.5| >= 2^24.  Differentiable
    in tex (a shared texture's gradient sums over the batch) and uv.

    filter_mode "linear" (uv_da must be None) is the plain bilinear lookup.  "linear-mipmap-linear" prefilters: it
    needs uv_da [B,H,W,4] float32, (du/dX, du/dY, dv/dX, dv/dY) per step of one output pixel (attribute_derivatives()
    computes it for a rasterized mesh), builds the pyramid of texture_mip_levels(Ht, Wt, max_mip_level) levels (each
    the 2 x 2 box filter of the one below, while both extents are even), takes lod = log2 of the longer pixel
    footprint axis in level-0 texels, clamped to the pyramid, and blends the bilinear lookups of levels floor(lod)
    and floor(lod) + 1.  The gradient to tex spreads over the whole footprint.  uv_da and mask get no gradient: the
    level of detail is a filter-width decision and is treated as a constant.  With uv_da all zero the result equals
    the "linear" one bit for bit.  Full statement: INTEGRATION.md, "Texture mapping"."""
    _check_texture_args(tex, uv, mask, boundary_mode)
    _check_filter_args(filter_mode, max_mip_level)
    if filter_mode == "linear":
        if uv_da is not None:
            raise ValueError("uv_da is only used with filter_mode='linear-mipmap-linear'.")
        return TextureSample.apply(tex, uv, mask, boundary_mode)
    if uv_da is None:
        raise ValueError("filter_mode='linear-mipmap-linear' requires uv_da.")
    if not torch.is_tensor(uv_da) or list(uv_da.shape) != list(uv.shape[:3]) + [4] or uv_da.dtype != torch.float32:
        raise ValueError("uv_da must be a float32 tensor of shape [batch_size, height, width, 4] matching uv.")
    return TextureMipSample.apply(tex, uv, uv_da, mask, boundary_mode, max_mip_level)


def render_textured(vertices, triangles, uvs, texture, camera_position, camera_lookat, camera_up, image_width,
                    image_height, uv_triangles=None, normals=None, sh_coefficients=None, fov_y=40.0,
                    near_clip=0.01, far_clip=10.0, boundary_mode="wrap", antialias=False):
    """Render a batch of textured meshes with bilinear texture filtering; returns [B,H,W,4] RGBA, row 0 at the top.
    render_textured_filtered(..., filter_mode="linear") under its pinned signature: see there."""
    return render_textured_filtered(vertices, triangles, uvs, texture, camera_position, camera_lookat, camera_up,
                                    image_width, image_height, uv_triangles=uv_triangles, normals=normals,
                                    sh_coefficients=sh_coefficients, fov_y=fov_y, near_clip=near_clip,
                                    far_clip=far_clip, boundary_mode=boundary_mode, antialias=antialias)


def render_textured_filtered(vertices, triangles, uvs, texture, camera_position, camera_lookat, camera_up, image_width,
                             image_height, uv_triangles=None, normals=None, sh_coefficients=None, fov_y=40.0,
                             near_clip=0.01, far_clip=10.0, boundary_mode="wrap", antialias=False,
                             filter_mode="linear", max_mip_level=None):
    """Render a batch of textured meshes; returns [B,H,W,4] RGBA, row 0 at the top.

    vertices [B,V,3], triangles [T,3] int32 (clockwise winding faces the viewer), camera_* [B,3] or [3], fov_y,
    near_clip, far_clip float, 0-D or [B], as in render_sh().  uvs [Vt,2] or [B,Vt,2]: texture coordinates,
    indexed corner by corner through uv_triangles [T,3] int32 (the same triangles in the same order), or per
    vertex through `triangles` when uv_triangles is None (then Vt = V).  texture [Ht,Wt,3] or [B,Ht,Wt,3]: the
    RGB albedo, sampled as texture() does with `boundary_mode`.  With sh_coefficients None the albedo is the
    colour (unlit); otherwise rgb = albedo * SH irradiance by sh_shader()'s rule, which needs per-vertex
    normals [B,V,3].  alpha is the coverage (fractional on the outline with antialias=True); rgb is 0 on the
    background.  filter_mode "linear-mipmap-linear" samples with mipmapped trilinear filtering (texture_filtered()), the
    level of detail from the analytic screen-space UV derivatives of the rasterized mesh (attribute_derivatives(),
    not differentiated); max_mip_level caps the pyramid.  Differentiable in vertices, uvs, texture, normals,
    sh_coefficients and device cameras."""
    if len(vertices.shape) != 3 or vertices.shape[-1] != 3:
        raise ValueError("Vertices must have shape [batch_size, vertex_count, 3].")
    batch_size, vertex_count = vertices.shape[0], vertices.shape[1]
    device = vertices.device
    if not torch.is_tensor(triangles) or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError("Triangles must have shape [triangle_count, 3].")
    if not torch.is_tensor(uvs) or uvs.dim() not in (2, 3) or uvs.shape[-1] != 2 or (
            uvs.dim() == 3 and uvs.shape[0] != batch_size):
        raise ValueError("uvs must have shape [uv_count, 2] or [batch_size, uv_count, 2].")
    if uv_triangles is not None:
        if not torch.is_tensor(uv_triangles) or list(uv_triangles.shape) != list(triangles.shape):
            raise ValueError("uv_triangles must have shape [triangle_count, 3], like triangles.")
        if uv_triangles.dtype != torch.int32:
            raise ValueError("uv_triangles must be int32.")
        _check_corner_indices(uv_triangles, uvs.shape[-2])
    elif uvs.shape[-2] != vertex_count:
        raise ValueError("uvs must have one row per vertex when uv_triangles is None.")
    if not torch.is_tensor(texture) or texture.dim() not in (3, 4) or (
            texture.dim() == 4 and texture.shape[0] != batch_size):
        raise ValueError("texture must have shape [Ht, Wt, 3] or [batch_size, Ht, Wt, 3].")
    if texture.shape[-1] != 3:
        raise ValueError("texture must have 3 channels (RGB albedo), got %d." % texture.shape[-1])
    if boundary_mode not in _BOUNDARY_MODES:
        raise ValueError("boundary_mode must be 'wrap' or 'clamp', got %r." % (boundary_mode,))
    _check_filter_args(filter_mode, max_mip_level)
    sh = None
    if sh_coefficients is not None:
        if normals is None:
            raise ValueError("normals are required with sh_coefficients.")
        if len(normals.shape) != 3 or normals.shape[-1] != 3 or list(normals.shape[:2]) != [batch_size,
                                                                                               vertex_count]:
            raise ValueError("Normals must have shape [batch_size, vertex_count, 3].")
        sh = _sh_batch(sh_coefficients, batch_size, device)
    camera_position = _per_batch_vec3(camera_position, batch_size, "camera_position")
    camera_lookat = _per_batch_vec3(camera_lookat, batch_size, "camera_lookat")
    if list(camera_up.shape) == [3]:
        camera_up = camera_up.unsqueeze(0).repeat(batch_size, 1)
    elif list(camera_up.shape) != [batch_size, 3]:
        raise ValueError("camera_up must have shape [batch_size, 3] or [3].")
    fov_y = _per_batch(fov_y, batch_size, camera_position.device, "fov_y")
    near_clip = _per_batch(near_clip, batch_size, camera_position.device, "near_clip")
    far_clip = _per_batch(far_clip, batch_size, camera_position.device, "far_clip")

    from .rasterize_triangles_ext import AttributeInterpolator, BarycentricRasterizer
    clip_space_transforms = camera_utils.clip_space_transforms(
        camera_position, camera_lookat, camera_up, fov_y, near_clip, far_clip, image_width / image_height, device)
    clip = camera_utils.transform_homogeneous(clip_space_transforms, vertices)
    ids, bary, z = BarycentricRasterizer.apply(clip, triangles, image_width, image_height)
    # (u, v, 1) per corner, background 0: the third channel is 0 off the mesh and sum(bary) (1 within rounding) on it
    if uvs.dim() == 2:
        uvs = uvs.unsqueeze(0).expand(batch_size, uvs.shape[0], 2)
    uvs = uvs.to(device)
    ones = torch.ones(batch_size, uvs.shape[1], 1, dtype=uvs.dtype, device=device)
    uv_attributes = torch.cat([uvs, ones], 2)
    corner_triangles = uv_triangles.to(device) if uv_triangles is not None else triangles
    pixel_uv = AttributeInterpolator.apply(ids, bary, uv_attributes, corner_triangles,
                                           torch.zeros(3, device=device))
    alpha = (pixel_uv[..., 2].detach() > 0.5).to(torch.float32)   # the coverage, exactly 1 or 0
    if filter_mode == "linear":
        albedo = TextureSample.apply(texture.to(device), pixel_uv[..., 0:2].contiguous(), alpha, boundary_mode)
    else:
        uv_da = _native.attribute_derivatives(ids, bary.detach(), clip.detach(), triangles, uvs.detach().contiguous(),
                                              corner_triangles if uv_triangles is not None else None)
        albedo = TextureMipSample.apply(texture.to(device), pixel_uv[..., 0:2].contiguous(),
                                        uv_da.view(batch_size, image_height, image_width, 4), alpha, boundary_mode,
                                        max_mip_level)
    if sh is not None:
        pixel_normals = AttributeInterpolator.apply(ids, bary, normals, triangles, torch.zeros(3, device=device))
        image = SHShade.apply(pixel_normals, albedo, alpha, sh, not antialias)
        if not antialias:
            return image
    else:
        image = torch.cat([albedo, alpha.unsqueeze(3)], 3)
    if antialias:
        from .antialiasing import antialias as antialias_op
        image = antialias_op(image, clip, triangles, ids, bary, z)
    return torch.flip(image, dims=[1])
