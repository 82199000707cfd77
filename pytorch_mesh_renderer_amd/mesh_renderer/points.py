"""Point-cloud losses: nearest neighbours, Chamfer distance and area-weighted surface sampling.

The data term for fitting a mesh to 3D data -- a scan, a depth camera's point cloud, another mesh -- next to the
regularisers of mesh_renderer.regularizers ("Point-cloud losses").  On a HIP device the float32
clouds go through csrc/nearest.hip: a brute-force nearest-neighbour search that never forms the N x M distance
tensor, a fixed-order mean, and a backward without atomics (a gather over an inverted index of the saved
neighbours), bitwise reproducible in either deterministic mode.  Host tensors and tensors that are not float32 --
data preparation, the CPU test-suite -- take the equivalent torch expression, chunked over the queries.
Distances are always computed as (x - y).(x - y), never as |x|^2 + |y|^2 - 2 x.y.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _native

_CHUNK_BYTES = 64 << 20   # the torch spelling never forms more than about this much at once


def _cloud(name, t):
    if not torch.is_tensor(t) or not t.is_floating_point():
        raise TypeError("%s must be a floating-point tensor" % name)
    if t.dim() not in (2, 3) or t.shape[-1] != 3 or t.shape[-2] < 1:
        raise ValueError("%s must have shape [B, N, 3] or [N, 3] with N >= 1, got %s" % (name, list(t.shape)))


def _lengths(name, lengths, B, limit, like):
    """-> int32 [B] on the clouds' device, clamped to [0, limit] on the device (no host synchronisation), or None."""
    if lengths is None:
        return None
    if not torch.is_tensor(lengths):
        raise TypeError("%s must be an integer tensor" % name)
    if lengths.is_floating_point() or lengths.is_complex() or lengths.dtype == torch.bool:
        raise RuntimeError("%s must hold integer point counts" % name)
    if lengths.dim() != 1 or lengths.shape[0] != B:
        raise ValueError("%s must have shape [%d], got %s" % (name, B, list(lengths.shape)))
    if lengths.device != like.device:
        raise RuntimeError("%s must be on the clouds' device" % name)
    return lengths.clamp(0, limit).to(torch.int32)


def _arguments(x, y, x_lengths, y_lengths):
    """-> (x [B,N,3], y [B,M,3], x_lengths, y_lengths, whether the clouds came without the batch axis)."""
    _cloud("x", x)
    _cloud("y", y)
    if x.dim() != y.dim():
        raise ValueError("x and y must both have a batch axis or both lack it, got %s and %s"
                         % (list(x.shape), list(y.shape)))
    single = x.dim() == 2
    if single:
        x, y = x.unsqueeze(0), y.unsqueeze(0)
    if x.shape[0] != y.shape[0] or x.shape[0] < 1:
        raise ValueError("x and y must have the same batch size, got %s and %s" % (list(x.shape), list(y.shape)))
    if x.device != y.device:
        raise RuntimeError("x and y must be on the same device")
    if x.dtype != y.dtype:
        raise RuntimeError("x and y must have the same dtype, got %s and %s" % (x.dtype, y.dtype))
    if single:
        x_lengths = x_lengths.reshape(1) if torch.is_tensor(x_lengths) and x_lengths.dim() == 0 else x_lengths
        y_lengths = y_lengths.reshape(1) if torch.is_tensor(y_lengths) and y_lengths.dim() == 0 else y_lengths
    B = x.shape[0]
    return (x, y, _lengths("x_lengths", x_lengths, B, x.shape[1], x), _lengths("y_lengths", y_lengths, B, y.shape[1], x),
            single)


def _on_hip_path(x):
    return x.is_cuda and x.dtype == torch.float32


class _Nearest(torch.autograd.Function):
    """Both public functions on the HIP path.  reduce False: (sqdist [B,N], idx [B,N]) of x -> y.  reduce True:
    x_weight * mean_i sqdist(x -> y) + y_weight * mean_j sqdist(y -> x) per image [B]; a direction whose weight is
    0 does not run."""

    @staticmethod
    def forward(ctx, x, y, x_lengths, y_lengths, x_weight, y_weight, reduce):
        xd, yd = x.detach().contiguous(), y.detach().contiguous()
        ctx.reduce, ctx.weights = reduce, (x_weight, y_weight)
        if not reduce:
            sqdist, idx, _ = _native.nearest_forward(xd, yd, x_lengths, y_lengths)
            ctx.directions = (True, False)
            ctx.save_for_backward(xd, yd, x_lengths, y_lengths, idx, None)
            ctx.mark_non_differentiable(idx)
            return sqdist, idx
        idx_xy = idx_yx = None
        total = True
        if x_weight != 0.0:
            _, idx_xy, total = _native.nearest_forward(xd, yd, x_lengths, y_lengths, want_sqdist=False, total=total,
                                                       weight=x_weight)
        if y_weight != 0.0:
            _, idx_yx, total = _native.nearest_forward(yd, xd, y_lengths, x_lengths, want_sqdist=False, total=total,
                                                       weight=y_weight)
        if total is True:   # both weights 0
            total = torch.zeros(xd.shape[0], dtype=torch.float32, device=xd.device)
        ctx.directions = (idx_xy is not None, idx_yx is not None)
        ctx.save_for_backward(xd, yd, x_lengths, y_lengths, idx_xy, idx_yx)
        return total

    @staticmethod
    @once_differentiable
    def backward(ctx, grad, _unused=None):
        x, y, x_lengths, y_lengths, idx_xy, idx_yx = ctx.saved_tensors
        want_dx, want_dy = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        none = (None,) * 5
        if not (want_dx or want_dy):
            return (None, None) + none
        if not any(ctx.directions):
            return (torch.zeros_like(x) if want_dx else None, torch.zeros_like(y) if want_dy else None) + none
        # a cloud's gradient needs the inverted index of the direction that ran INTO it, and nothing else is built
        index_xy = _inverted_index(idx_xy, y.shape[1]) if want_dy and idx_xy is not None else None
        index_yx = _inverted_index(idx_yx, x.shape[1]) if want_dx and idx_yx is not None else None
        grad = grad.contiguous()
        dx, dy = _native.nearest_backward(
            x, y, x_lengths, y_lengths, idx_xy, index_xy, idx_yx, index_yx,
            grad_points=None if ctx.reduce else grad, grad_images=grad if ctx.reduce else None,
            x_weight=ctx.weights[0], y_weight=ctx.weights[1], want_dx=want_dx, want_dy=want_dy)
        return (dx, dy) + none


def _inverted_index(idx, targets):
    return _native.nearest_inverted_index(idx, targets)


def _nearest_torch(x, y, x_lengths, y_lengths):
    """nearest_points as a torch expression on the device and in the dtype of x [B,N,3] / y [B,M,3]: the neighbour is
    searched chunk by chunk of queries without a graph, the distance to it is then an ordinary differentiable
    gather."""
    B, N, _ = x.shape
    M = y.shape[1]
    dev = x.device
    n_valid = x_lengths.long() if x_lengths is not None else torch.full((B,), N, dtype=torch.int64, device=dev)
    m_valid = y_lengths.long() if y_lengths is not None else torch.full((B,), M, dtype=torch.int64, device=dev)
    outside = torch.arange(M, device=dev)[None, None, :] >= m_valid[:, None, None]          # [B,1,M]
    rows = max(1, _CHUNK_BYTES // max(1, B * M * 3 * x.element_size()))
    found = []
    with torch.no_grad():
        for start in range(0, N, rows):
            diff = x[:, start:start + rows, None, :] - y[:, None, :, :]
            d = (diff * diff).sum(-1).masked_fill(outside, float("inf"))
            found.append(d.min(dim=2).indices)   # the first of equal minima
        idx = torch.cat(found, dim=1)
    valid = (torch.arange(N, device=dev)[None, :] < n_valid[:, None]) & (m_valid > 0)[:, None]
    idx = torch.where(valid, idx, torch.full_like(idx, -1))
    chosen = torch.gather(y, 1, idx.clamp(min=0)[..., None].expand(-1, -1, 3))
    diff = torch.where(valid[..., None], x - chosen, torch.zeros_like(x))   # padded rows: value 0, gradient 0
    return (diff * diff).sum(-1), idx.to(torch.int32)


def _mean_torch(sqdist, lengths, other_lengths):
    """The mean of sqdist [B,N] over the valid queries (padded rows are 0 already); 0 where either side is empty."""
    B, N = sqdist.shape
    if lengths is None:
        count = torch.full((B,), float(N), dtype=sqdist.dtype, device=sqdist.device)
    else:
        count = lengths.to(sqdist.dtype)
    mean = sqdist.sum(1) / count.clamp(min=1)
    if other_lengths is not None:
        mean = torch.where(other_lengths > 0, mean, torch.zeros_like(mean))
    return mean


def nearest_points(x, y, x_lengths=None, y_lengths=None):
    """x [B,N,3], y [B,M,3] (or [N,3], [M,3]: one image, results without the batch axis) -> (sqdist [B,N], idx [B,N]
    int32): for every x[b,i] the squared Euclidean distance to its nearest y[b,j] with j < y_lengths[b], and that j
    (the lowest of equally near ones).  sqdist is differentiable in x and y; idx is not.

    x_lengths, y_lengths: optional integer [B] tensors on the clouds' device for padded clouds, clamped to [0, N] /
    [0, M] on the device (nothing is read back to validate them).  A padded query row (i >= x_lengths[b]) and every
    query of an image whose target is empty get sqdist 0, idx -1 and no gradient; padded coordinates influence
    nothing.  Every other idx lies in [0, y_lengths[b]) even where coordinates are NaN or infinite."""
    x, y, x_lengths, y_lengths, single = _arguments(x, y, x_lengths, y_lengths)
    if _on_hip_path(x):
        sqdist, idx = _Nearest.apply(x, y, x_lengths, y_lengths, 1.0, 0.0, False)
    else:
        sqdist, idx = _nearest_torch(x, y, x_lengths, y_lengths)
    return (sqdist[0], idx[0]) if single else (sqdist, idx)


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_weight=1.0, y_weight=1.0):
    """x_weight * mean_i min_j |x_i - y_j|^2 + y_weight * mean_j min_i |x_i - y_j|^2 per image -> [B] (a 0-dim tensor
    for [N,3] / [M,3] clouds).  The means run over the valid points of each image (x_lengths, y_lengths as in
    nearest_points); a direction with an empty side contributes 0.  The weights are Python numbers; a direction whose
    weight is 0 is not computed, which gives the single-directional form.  Differentiable in x and y; on a HIP device
    both directions share one backward call, and a gradient that is not required is not computed."""
    x, y, x_lengths, y_lengths, single = _arguments(x, y, x_lengths, y_lengths)
    x_weight, y_weight = float(x_weight), float(y_weight)
    if _on_hip_path(x):
        total = _Nearest.apply(x, y, x_lengths, y_lengths, x_weight, y_weight, True)
    else:
        total = x.new_zeros(x.shape[0])
        if x_weight != 0.0:
            total = total + x_weight * _mean_torch(_nearest_torch(x, y, x_lengths, y_lengths)[0], x_lengths, y_lengths)
        if y_weight != 0.0:
            total = total + y_weight * _mean_torch(_nearest_torch(y, x, y_lengths, x_lengths)[0], y_lengths, x_lengths)
    return total[0] if single else total


def _mesh(vertices, triangles):
    if not torch.is_tensor(vertices) or not vertices.is_floating_point():
        raise TypeError("vertices must be a floating-point tensor")
    single = vertices.dim() == 2
    v = vertices.unsqueeze(0) if single else vertices
    if v.dim() != 3 or v.shape[2] != 3 or v.shape[1] < 1 or v.shape[0] < 1:
        raise ValueError("vertices must have shape [B, V, 3] or [V, 3] with V >= 1, got %s" % list(vertices.shape))
    if not torch.is_tensor(triangles):
        raise TypeError("triangles must be a tensor")
    if triangles.dtype in (torch.float16, torch.float32, torch.float64, torch.bfloat16, torch.bool):
        raise RuntimeError("triangles must hold integer vertex indices")
    if triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.shape[0] < 1:
        raise ValueError("triangles must have shape [T, 3] with T >= 1, got %s" % list(triangles.shape))
    return v, triangles.to(v.device).long(), single


def sample_surface_points_from_uniforms(vertices, triangles, uniforms, return_faces=False):
    """The deterministic core of sample_surface_points: vertices [B,V,3] (or [V,3]), triangles [T,3] of any integer
    dtype (one topology for the batch), uniforms [B,count,3] (or [count,3]) in [0, 1) -> points [B,count,3].

    The face is chosen from the cumulative face areas by uniforms[..., 0] (area-weighted; a zero-area face, or one
    with an index outside [0, V), is never chosen); the barycentrics are (1 - sqrt(u1), sqrt(u1) (1 - u2),
    sqrt(u1) u2).  The face choice is not differentiable; the points are differentiable to the vertices.  A mesh of
    total area 0 raises ValueError (this reads one flag back from the device).  With return_faces also the face ids
    [B,count] (int64) and the barycentrics [B,count,3].

    Batched torch ops on the vertices' device, O(count), no kernel of its own.  The backward is torch's index_add,
    so it is bit-reproducible only under torch's own switch, torch.use_deterministic_algorithms(True) --
    _native.set_deterministic does not reach it."""
    v, tris, single = _mesh(vertices, triangles)
    if not torch.is_tensor(uniforms) or not uniforms.is_floating_point():
        raise TypeError("uniforms must be a floating-point tensor")
    u = uniforms.unsqueeze(0) if single and uniforms.dim() == 2 else uniforms
    B, V, _ = v.shape
    if u.dim() != 3 or u.shape[0] != B or u.shape[2] != 3:
        raise ValueError("uniforms must have shape [%d, count, 3], got %s" % (B, list(uniforms.shape)))
    if u.device != v.device:
        raise RuntimeError("uniforms must be on the vertices' device")
    T = tris.shape[0]
    with torch.no_grad():
        usable = ((tris >= 0) & (tris < V)).all(dim=1)                       # [T]
        safe = tris.clamp(0, V - 1)
        corners = v.detach().double().index_select(1, safe.reshape(-1)).reshape(B, T, 3, 3)
        normal = torch.cross(corners[:, :, 1] - corners[:, :, 0], corners[:, :, 2] - corners[:, :, 0], dim=-1)
        areas = 0.5 * normal.norm(dim=-1) * usable[None, :]
        areas = torch.where(torch.isfinite(areas), areas, torch.zeros_like(areas))
        cumulative = areas.cumsum(1)                                          # [B,T] float64
        total = cumulative[:, -1:]
        if bool((total <= 0).any()):
            raise ValueError("a mesh of total area 0 has no surface to sample")
        wanted = (u[..., 0].double().clamp(0, 1) * total).contiguous()
        # the first face whose cumulative area EXCEEDS the value: a zero-area face's interval is empty
        face = torch.searchsorted(cumulative, wanted, right=True)
        positive = areas > 0
        last = (T - 1) - positive.flip(1).to(torch.int32).argmax(dim=1)        # the last face with an area
        face = torch.minimum(face, last[:, None])
    root = u[..., 1].clamp(0, 1).sqrt()
    bary = torch.stack([1.0 - root, root * (1.0 - u[..., 2]), root * u[..., 2]], dim=-1).to(v.dtype)
    which = safe[face] + (torch.arange(B, device=v.device) * V)[:, None, None]           # [B,count,3] rows of [B*V,3]
    picked = v.reshape(B * V, 3).index_select(0, which.reshape(-1)).reshape(B, -1, 3, 3)
    points = (bary[..., None] * picked).sum(2)
    if single:
        points, face, bary = points[0], face[0], bary[0]
    return (points, face, bary) if return_faces else points


def sample_surface_points(vertices, triangles, count, generator=None, return_faces=False):
    """`count` points per image, uniformly distributed over the surface of the mesh (area-weighted) -> [B,count,3]
    (or [count,3] for [V,3] vertices): sample_surface_points_from_uniforms on torch.rand numbers drawn from
    `generator` (on the generator's device; the default generator of the vertices' device without one).  The points
    are differentiable to the vertices through torch's index_add (bit-reproducible only under
    torch.use_deterministic_algorithms(True)); which face a point lands on is not differentiable.  With return_faces
    also the face ids and barycentrics."""
    v, _, single = _mesh(vertices, triangles)
    count = int(count)
    if count < 1:
        raise ValueError("count must be at least 1, got %d" % count)
    where = generator.device if generator is not None else v.device
    uniforms = torch.rand(v.shape[0], count, 3, generator=generator, device=where, dtype=torch.float32).to(v.device)
    if single:
        uniforms = uniforms[0]
    return sample_surface_points_from_uniforms(vertices, triangles, uniforms, return_faces=return_faces)
