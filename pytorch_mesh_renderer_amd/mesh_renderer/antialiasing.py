"""Differentiable analytic antialiasing of silhouette edges for the hard rasterizer.

The hard rasterizer's image has a binary alpha: nothing in a pixel on an object's outline depends
continuously on where the outline lies, so a loss on the outline has no gradient to the vertices.
antialias() blends each pair of neighbouring pixels that a silhouette edge separates by where the edge
crosses the segment between the two pixel centres, and differentiates that crossing point with respect to
the edge's clip-space vertices (in the style of Laine et al. 2020, "Modular Primitives for High-Performance
Differentiable Rendering").  The full semantics are in INTEGRATION.md, "Silhouette antialiasing"; the HIP
kernels are csrc/antialias.hip.
"""
import torch

from .. import _native


def antialias_topology(triangles, vertex_count):
    """[T,3] int32 triangles -> opposite [T,3] int32 on the same device: for the edge opposite corner k of
    triangle t, the neighbouring triangle's vertex across that edge; -1 for a boundary edge, -2 for a
    non-manifold or degenerate one.  Cached on the tensor (recomputed after an in-place write)."""
    if not torch.is_tensor(triangles) or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [triangle_count, 3].")
    if triangles.dtype != torch.int32:
        raise ValueError("triangles must be int32, got %s." % str(triangles.dtype).replace("torch.", ""))
    return _native.antialias_topology(triangles, int(vertex_count))


def _check(image, clip_space_vertices, triangles, triangle_ids, barycentrics, z, topology):
    named = (("image", image), ("clip_space_vertices", clip_space_vertices), ("triangles", triangles),
             ("triangle_ids", triangle_ids), ("barycentrics", barycentrics), ("z", z))
    for name, t in named:
        if not torch.is_tensor(t):
            raise ValueError("%s must be a tensor." % name)
    if image.dim() != 4 or image.shape[3] < 1:
        raise ValueError("image must have shape [batch_size, height, width, channels], channels >= 1.")
    B, H, W, _ = image.shape
    if clip_space_vertices.dim() != 3 or clip_space_vertices.shape[0] != B or clip_space_vertices.shape[2] != 4:
        raise ValueError("clip_space_vertices must have shape [batch_size, vertex_count, 4].")
    if triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [triangle_count, 3].")
    if list(triangle_ids.shape) != [B, H, W]:
        raise ValueError("triangle_ids must have shape [batch_size, height, width] matching the image.")
    if list(barycentrics.shape) != [B, H, W, 3]:
        raise ValueError("barycentrics must have shape [batch_size, height, width, 3] matching the image.")
    if list(z.shape) != [B, H, W]:
        raise ValueError("z must have shape [batch_size, height, width] matching the image.")
    if topology is not None and list(topology.shape) != [triangles.shape[0], 3]:
        raise ValueError("topology must have shape [triangle_count, 3].")
    for name, t, want in (("image", image, torch.float32), ("clip_space_vertices", clip_space_vertices, torch.float32),
                          ("triangles", triangles, torch.int32), ("triangle_ids", triangle_ids, torch.int32),
                          ("barycentrics", barycentrics, torch.float32), ("z", z, torch.float32),
                          ("topology", topology, torch.int32)):
        if t is not None and t.dtype != want:
            raise ValueError("%s must be %s, got %s." % (name, str(want).replace("torch.", ""),
                                                          str(t.dtype).replace("torch.", "")))
    devices = {t.device for _, t in named} | ({topology.device} if topology is not None else set())
    if len(devices) != 1:
        raise ValueError("all inputs of antialias must be on one device, got %s." % sorted(str(d) for d in devices))


class Antialias(torch.autograd.Function):
    """antialias() as one autograd op: forward and backward are single HIP passes over the image."""

    @staticmethod
    def forward(ctx, image, clip_space_vertices, triangles, triangle_ids, barycentrics, z, topology):
        image, clip = image.detach(), clip_space_vertices.detach()
        out = _native.antialias_forward(image, triangle_ids, barycentrics.detach(), z.detach(), clip, triangles,
                                        topology)
        ctx.save_for_backward(image, clip, triangles, triangle_ids, barycentrics.detach(), z.detach(), topology)
        return out

    @staticmethod
    def backward(ctx, dout):
        image, clip, triangles, ids, bary, z, topology = ctx.saved_tensors
        dimage, dclip = _native.antialias_backward(dout.contiguous(), image, ids, bary, z, clip, triangles, topology)
        return (dimage if ctx.needs_input_grad[0] else None, dclip if ctx.needs_input_grad[1] else None,
                None, None, None, None, None)


def antialias(image, clip_space_vertices, triangles, triangle_ids, barycentrics, z, topology=None):
    """Antialias the silhouette edges of a rasterized image; differentiable in image and clip_space_vertices.

    image [B,H,W,C] f32 (any C >= 1) and the G-buffer triangle_ids [B,H,W] i32, barycentrics [B,H,W,3] f32,
    z [B,H,W] f32 that rasterize_barycentric returned for clip_space_vertices [B,V,4] f32 and triangles
    [T,3] i32, all in the rasterizer's row order (row 0 = bottom scanline).  topology: the mesh's
    antialias_topology(triangles, V), computed (and cached on `triangles`) when None.

    A pixel is covered iff its id != 0 or (b0 + b1) + b2 >= 0.9.  Each horizontal and vertical pair of
    neighbouring pixels whose ids differ, or of which exactly one is covered, is considered once: the front
    pixel f (the covered one; else the smaller z; else the larger id) lies in triangle F, and the segment
    from f to the other pixel g leaves F through its edge i with the smallest t = e_i(f) / (e_i(f) - e_i(g))
    among the edges with e_i(g) < 0.  If that edge is a silhouette (no neighbour, non-manifold, or the
    neighbour folds away from the viewer) the pixel on the far side of the midpoint from the edge takes
    |t - 0.5| of the other pixel's colour: out[g] += (t - 0.5)(c_f - c_g) for t > 0.5, out[f] +=
    (0.5 - t)(c_g - c_f) for t < 0.5.  The gradient of t reaches the edge's two vertices' clip x, y, w.
    Edges of triangles with a vertex at w <= 0 are not antialiased; seams with duplicated vertices blend like
    outlines.  Full statement: INTEGRATION.md, "Silhouette antialiasing"."""
    _check(image, clip_space_vertices, triangles, triangle_ids, barycentrics, z, topology)
    if topology is None:
        topology = antialias_topology(triangles, clip_space_vertices.shape[1])
    return Antialias.apply(image, clip_space_vertices, triangles, triangle_ids, barycentrics, z, topology)
