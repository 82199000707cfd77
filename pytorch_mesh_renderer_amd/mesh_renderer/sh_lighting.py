"""Differentiable diffuse shading under second-order spherical-harmonics (SH) environment lighting.

Point lights enter a loss non-linearly through their positions; SH irradiance is linear in 27 numbers per image,
which makes fitting the lighting of a photograph a well-conditioned least-squares problem inside the same
optimisation as the geometry.  sh_shader() is the pixel-buffer op (the SH counterpart of phong_shader) and
render_sh() the whole render.  The semantics are in INTEGRATION.md, "Spherical-harmonics lighting"; the HIP
kernels are csrc/sh_shade.hip.
"""
import torch

from .. import _native
from ..common import camera_utils
from .rasterize import rasterize
from .render import _per_batch, _per_batch_vec3

# True: sh_shader() and render_sh() shade with the HIP kernels.  False: with the torch restatement below -- the
# same results within float32 rounding, kept as a cross-check (tests).  Read at call time, like
# render.USE_FUSED_SHADING.
USE_SH_KERNELS = True

_SH_SHAPE_ERROR = "sh_coefficients must have shape [batch_size, 9, 3] or [9, 3]."


def _sh_batch(sh_coefficients, batch_size, device):
    """[9,3] or [B,9,3] -> [B,9,3] on `device` (a [9,3] argument is broadcast, its gradient summed)."""
    if not torch.is_tensor(sh_coefficients):
        raise ValueError(_SH_SHAPE_ERROR)
    if list(sh_coefficients.shape) == [9, 3]:
        sh_coefficients = sh_coefficients.unsqueeze(0).expand(batch_size, 9, 3)
    elif list(sh_coefficients.shape) != [batch_size, 9, 3]:
        raise ValueError(_SH_SHAPE_ERROR)
    return sh_coefficients.to(device)


def _sh_rgba_torch(normals, alphas, diffuse_colors, sh):
    """The torch restatement of the kernels, rows in the input's order.  alphas None: derived from the diffuse
    colours (any channel >= 0), without gradient."""
    if alphas is None:
        alphas = (diffuse_colors >= 0.0).any(dim=3).to(diffuse_colors.dtype)
    n = torch.nn.functional.normalize(normals, p=2, dim=3)
    x, y, z = n.unbind(3)
    basis = torch.stack([torch.full_like(x, 0.282094791773878), 0.488602511902920 * y, 0.488602511902920 * z,
                         0.488602511902920 * x, 1.092548430592079 * x * y, 1.092548430592079 * y * z,
                         0.315391565252520 * (3.0 * z * z - 1.0), 1.092548430592079 * x * z,
                         0.546274215296040 * (x * x - y * y)], dim=3)
    irradiance = torch.einsum("bhwk,bkc->bhwc", basis, sh)
    rgb = diffuse_colors * irradiance
    alpha = alphas.unsqueeze(3)
    rgb = torch.where(alpha > 0.5, rgb, torch.zeros_like(rgb))
    return torch.cat([rgb, alpha], dim=3)


class SHShade(torch.autograd.Function):
    """The SH shading of separate normal / diffuse / alpha buffers as one autograd op (one HIP pass each way)."""

    @staticmethod
    def forward(ctx, normals, diffuse_colors, alphas, sh, flip):
        normals, diffuse_colors, sh = normals.detach(), diffuse_colors.detach(), sh.detach()
        alphas = alphas.detach() if alphas is not None else None
        ctx.flip = flip
        ctx.has_alphas = alphas is not None
        ctx.save_for_backward(normals, diffuse_colors, alphas, sh)
        return _native.sh_shade_forward(normals, diffuse_colors, alphas, sh, flip=flip)

    @staticmethod
    def backward(ctx, drgba):
        normals, diffuse_colors, alphas, sh = ctx.saved_tensors
        need = ctx.needs_input_grad
        dnormals, ddiffuse, dalphas, dsh = _native.sh_shade_backward(
            drgba, normals, diffuse_colors, alphas, sh, flip=ctx.flip, want_normals=need[0], want_diffuse=need[1],
            want_alphas=ctx.has_alphas and need[2], want_sh=need[3])
        return dnormals, ddiffuse, dalphas, dsh, None


class SHShadePacked(torch.autograd.Function):
    """SH shading of rasterize()'s packed [B,H,W,6] = [normals, diffuse] buffer, alpha derived from the diffuse
    colours: the kernels read the two slices in place, and the backward returns the packed gradient in one write
    (autograd's slice backward would cost two more full-image passes)."""

    @staticmethod
    def forward(ctx, attributes, sh, flip):
        attributes, sh = attributes.detach().contiguous(), sh.detach()
        ctx.flip = flip
        ctx.save_for_backward(attributes, sh)
        return _native.sh_shade_forward(attributes[..., 0:3], attributes[..., 3:6], None, sh, flip=flip)

    @staticmethod
    def backward(ctx, drgba):
        attributes, sh = ctx.saved_tensors
        normals, diffuse = attributes[..., 0:3], attributes[..., 3:6]
        want_sh = ctx.needs_input_grad[1]
        if not ctx.needs_input_grad[0]:
            dsh = _native.sh_shade_backward(drgba, normals, diffuse, None, sh, flip=ctx.flip, want_normals=False,
                                            want_diffuse=False, want_sh=want_sh)[3]
            return None, dsh, None
        dattributes, _, dsh = _native.sh_shade_backward(drgba, normals, diffuse, None, sh, flip=ctx.flip,
                                                        want_sh=want_sh, packed_grad=True)
        return dattributes, dsh, None


def _shade_packed(attributes, sh, flip):
    """[B,H,W,6] = [normals, diffuse] pixel attributes (background diffuse -1) -> RGBA."""
    if USE_SH_KERNELS:
        return SHShadePacked.apply(attributes, sh, flip)
    rgba = _sh_rgba_torch(attributes[..., 0:3], None, attributes[..., 3:6], sh)
    return torch.flip(rgba, dims=[1]) if flip else rgba


def sh_shader(normals, alphas, diffuse_colors, sh_coefficients):
    """Diffuse shading under second-order SH irradiance; returns [B,H,W,4] RGBA with row 0 at the top.

    normals [B,H,W,3] (normalised here), alphas [B,H,W] or None (then 1 where any diffuse channel is >= 0, as
    render() marks its background with -1), diffuse_colors [B,H,W,3], sh_coefficients [B,9,3] or [9,3]: per
    image nine real SH IRRADIANCE coefficients per RGB channel in world space (the cosine-lobe convolution is
    already folded in).  rgb = diffuse * sum_k sh[k] Y_k(n), not clamped, so the image is linear in the
    coefficients; rgb = 0 where alpha <= 0.5.  Differentiable in normals, diffuse_colors, sh_coefficients and
    alphas (which receive the alpha channel of the upstream gradient).  Full statement: INTEGRATION.md,
    "Spherical-harmonics lighting"."""
    if not torch.is_tensor(normals) or normals.dim() != 4 or normals.shape[3] != 3:
        raise ValueError("normals must have shape [batch_size, height, width, 3].")
    batch_size, height, width = normals.shape[:3]
    if not torch.is_tensor(diffuse_colors) or list(diffuse_colors.shape) != [batch_size, height, width, 3]:
        raise ValueError("diffuse_colors must have shape [batch_size, height, width, 3] matching the normals.")
    if alphas is not None and (not torch.is_tensor(alphas) or list(alphas.shape) != [batch_size, height, width]):
        raise ValueError("alphas must have shape [batch_size, height, width] matching the normals.")
    sh = _sh_batch(sh_coefficients, batch_size, normals.device)
    if USE_SH_KERNELS:
        return SHShade.apply(normals, diffuse_colors, alphas, sh, True)
    return torch.flip(_sh_rgba_torch(normals, alphas, diffuse_colors, sh), dims=[1])


def render_sh(vertices, triangles, normals, diffuse_colors, sh_coefficients, camera_position, camera_lookat,
              camera_up, image_width, image_height, fov_y=40.0, near_clip=0.01, far_clip=10.0, antialias=False):
    """Render a batch of meshes lit by second-order SH environment lighting; returns [B,H,W,4] RGBA, row 0 at
    the top, alpha in {0,1} (fractional on the outline with antialias=True).

    The arguments are render()'s without the lights and the specular term: vertices, normals and diffuse_colors
    [B,V,3], triangles [T,3] int32 (clockwise winding faces the viewer), camera_* [B,3] or [3], fov_y, near_clip,
    far_clip float, 0-D or [B]; sh_coefficients [B,9,3] or [9,3] as in sh_shader().  The per-vertex normals and
    diffuse colours are interpolated per pixel and shaded by sh_shader()'s rule.  antialias=True antialiases the
    silhouettes with mesh_renderer.antialias before the flip, as render(..., antialias=True) does."""
    if len(vertices.shape) != 3 or vertices.shape[-1] != 3:
        raise ValueError("Vertices must have shape [batch_size, vertex_count, 3].")
    batch_size = vertices.shape[0]
    device = vertices.device
    if len(normals.shape) != 3 or normals.shape[-1] != 3:
        raise ValueError("Normals must have shape [batch_size, vertex_count, 3].")
    if len(diffuse_colors.shape) != 3 or diffuse_colors.shape[-1] != 3:
        raise ValueError("diffuse_colors must have shape [batch_size, vertex_count, 3].")
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

    vertex_attributes = torch.cat([normals, diffuse_colors], 2)
    clip_space_transforms = camera_utils.clip_space_transforms(
        camera_position, camera_lookat, camera_up, fov_y, near_clip, far_clip, image_width / image_height, device)
    # background -1 marks uncovered pixels: a real diffuse colour is never negative
    background = torch.full((6,), -1.0, device=device)
    if not antialias:
        pixel_attributes = rasterize(vertices, vertex_attributes, triangles, clip_space_transforms,
                                     image_width, image_height, background)
        return _shade_packed(pixel_attributes, sh, True)
    # the composed ops of render(..., antialias=True): the G-buffer is handed on to the antialiasing pass
    from .antialiasing import antialias as antialias_op
    from .rasterize_triangles_ext import AttributeInterpolator, BarycentricRasterizer
    clip = camera_utils.transform_homogeneous(clip_space_transforms, vertices)
    ids, bary, z = BarycentricRasterizer.apply(clip, triangles, image_width, image_height)
    pixel_attributes = AttributeInterpolator.apply(ids, bary, vertex_attributes, triangles, background)
    image = antialias_op(_shade_packed(pixel_attributes, sh, False), clip, triangles, ids, bary, z)
    return torch.flip(image, dims=[1])
