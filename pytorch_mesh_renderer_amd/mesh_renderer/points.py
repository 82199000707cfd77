"""Point-cloud losses: nearest neighbours, Chamfer distance, point-to-mesh distance and area-weighted surface sampling.

The data term for fitting a mesh to 3D data -- a scan, a depth camera's point cloud, another mesh -- next to the
regularisers of mesh_renderer.regularizers ("Point-cloud losses").  On a HIP device the float32
clouds go through csrc/nearest.hip: a brute-force nearest-neighbour search that never forms the N x M distance
tensor, a fixed-order mean, and a backward without atomics (a gather over an inverted index of the saved
neighbours), bitwise reproducible in either deterministic mode.  Host tensors and tensors that are not float32 --
data preparation, the CPU test-suite -- take the equivalent torch expression, chunked over the queries.
Distances are always computed as (x - y).(x - y), never as |x|^2 + |y|^2 - 2 x.y.  nearest_triangles and
point_mesh_distance measure to the mesh's surface itself -- the nearest closed triangle -- with kernels of the same
file and the same split between the HIP and the torch path; triangle_nearest_points and mesh_point_distance are the
other direction, every triangle against its nearest point, and point_mesh_face_distance is the sum of the two means.
winding_number says on which side of the mesh a point lies -- the generalized winding number, an order-free fixed-point
sum over all triangles with kernels of the same file -- inside_mesh thresholds it, and signed_distance puts its sign
on nearest_triangles' distance.  cast_rays asks the sensor's question -- along this ray, where is the mesh first met? --
with the watertight test of Woop, Benthin and Wald in kernels of the same file, differentiable in the rays and the
vertices; rays_occluded is its yes or no.
knn_points is the K-neighbour form of nearest_points (a sorted list of K keys per query in registers, same file, same
split between the two paths), knn_gather reads values at its indices, and estimate_point_normals is its first
consumer: the normals of a scan from the covariance of every point's neighbourhood.  sample_farthest_points thins a
cloud to K well-spread points before any of these O(N M) searches (csrc/farthest.hip on a HIP device, a torch loop
of K steps elsewhere; both follow one bit-exact definition).  corresponding_points_alignment and
iterative_closest_point bring a scan that arrives in its sensor's frame -- rotated, shifted, at another scale -- into
the mesh's frame first: the least-squares similarity between matched points, and ICP around the module's own searches
against a cloud or against the mesh itself (csrc/align.hip; INTEGRATION.md, "Registration").
"""
import collections

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


# ---- K nearest neighbours ---------------------------------------------------------------------------------------------

class _Knn(torch.autograd.Function):
    """knn_points on the HIP path: (sqdist [B,N,K], idx [B,N,K]) of x -> y."""

    @staticmethod
    def forward(ctx, x, y, x_lengths, y_lengths, K):
        xd, yd = x.detach().contiguous(), y.detach().contiguous()
        sqdist, idx = _native.knn_forward(xd, yd, K, x_lengths, y_lengths)
        ctx.save_for_backward(xd, yd, x_lengths, y_lengths, sqdist, idx)
        ctx.mark_non_differentiable(idx)
        return sqdist, idx

    @staticmethod
    @once_differentiable
    def backward(ctx, grad, _unused=None):
        x, y, x_lengths, y_lengths, sqdist, idx = ctx.saved_tensors
        want_dx, want_dy = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        none = (None,) * 3
        if not (want_dx or want_dy):
            return (None, None) + none
        # the targets' gradient is a gather over the inverted index of the [B, N K] entries; nothing else needs it
        index = _inverted_index(idx.reshape(idx.shape[0], -1), y.shape[1]) if want_dy else None
        dx, dy = _native.knn_backward(x, y, x_lengths, y_lengths, sqdist, idx, grad.contiguous(), index,
                                      want_dx=want_dx, want_dy=want_dy)
        return (dx, dy) + none


def _knn_torch(x, y, K, x_lengths, y_lengths):
    """knn_points as a torch expression on the device and in the dtype of x [B,N,3] / y [B,M,3]: the neighbours are
    selected chunk by chunk of queries without a graph, by a stable sort of the distances (so equal distances go to
    the lowest index, NaN after every number, targets beyond y_lengths last); the distances to them are then an
    ordinary differentiable gather."""
    B, N, _ = x.shape
    M = y.shape[1]
    dev = x.device
    n_valid = x_lengths.long() if x_lengths is not None else torch.full((B,), N, dtype=torch.int64, device=dev)
    m_valid = y_lengths.long() if y_lengths is not None else torch.full((B,), M, dtype=torch.int64, device=dev)
    outside = torch.arange(M, device=dev)[None, None, :] >= m_valid[:, None, None]          # [B,1,M]
    rows = max(1, _CHUNK_BYTES // max(1, B * M * 3 * x.element_size()))
    kept = min(K, M)
    found = []
    with torch.no_grad():
        for start in range(0, N, rows):
            diff = x[:, start:start + rows, None, :] - y[:, None, :, :]
            d = (diff * diff).sum(-1).masked_fill(outside, float("nan"))
            found.append(torch.sort(d, dim=2, stable=True).indices[..., :kept])
        idx = torch.cat(found, dim=1)
        if kept < K:
            idx = torch.cat([idx, idx.new_zeros(B, N, K - kept)], dim=2)
        slot = torch.arange(K, device=dev)[None, None, :]
        valid = (torch.arange(N, device=dev)[None, :, None] < n_valid[:, None, None]) & (slot < m_valid[:, None, None])
        idx = torch.where(valid, idx, torch.full_like(idx, -1))
    diff = x[:, :, None, :] - knn_gather(y, idx)
    with torch.no_grad():
        finite = torch.isfinite((diff * diff).sum(-1))
    diff = torch.where((valid & finite)[..., None], diff, torch.zeros_like(diff))   # value 0, gradient 0
    sqdist = (diff * diff).sum(-1)
    sqdist = torch.where(valid & ~finite, torch.full_like(sqdist, float("inf")), sqdist)
    return sqdist, idx.to(torch.int32)


def knn_gather(values, idx):
    """values [B,M,C], idx [B,N,K] integer (or [M,C], [N,K]) -> [B,N,K,C]: values[b, idx[b,i,k]], zeros where idx is
    -1.  A torch gather: differentiable in values, and a slot with idx -1 passes no gradient."""
    if not torch.is_tensor(values) or not torch.is_tensor(idx):
        raise TypeError("values and idx must be tensors")
    if idx.is_floating_point() or idx.is_complex() or idx.dtype == torch.bool:
        raise RuntimeError("idx must hold integer indices")
    single = values.dim() == 2
    v, i = (values.unsqueeze(0), idx.unsqueeze(0)) if single else (values, idx)
    if v.dim() != 3 or i.dim() != 3 or v.shape[0] != i.shape[0]:
        raise ValueError("values must have shape [B, M, C] and idx [B, N, K] (or [M, C] and [N, K]), got %s and %s"
                         % (list(values.shape), list(idx.shape)))
    if v.device != i.device:
        raise RuntimeError("values and idx must be on the same device")
    B, N, K = i.shape
    C = v.shape[2]
    safe = i.long().clamp(0, v.shape[1] - 1)
    out = torch.gather(v, 1, safe.reshape(B, N * K, 1).expand(-1, -1, C)).reshape(B, N, K, C)
    out = torch.where((i >= 0)[..., None], out, torch.zeros_like(out))
    return out[0] if single else out


def knn_points(x, y, K, x_lengths=None, y_lengths=None, return_nn=False):
    """x [B,N,3], y [B,M,3] (or [N,3], [M,3]: one image, results without the batch axis), K a Python int in [1, 32]
    -> (sqdist [B,N,K], idx [B,N,K] int32[, nn [B,N,K,3] with return_nn]): for every x[b,i] its K nearest y[b,j]
    with j < y_lengths[b], nearest first, ordered by (squared Euclidean distance, j): equally distant targets come
    lowest index first.  sqdist (and nn = knn_gather(y, idx)) are differentiable in x and y; idx is not.

    x_lengths, y_lengths as in nearest_points.  A slot k >= y_lengths[b] (fewer than K targets) and every slot of a
    padded query row get sqdist 0, idx -1 and no gradient; padded coordinates influence nothing.  A distance that is
    NaN sorts after every number; its slot reports sqdist +inf with an idx in [0, y_lengths[b]), and a slot whose
    distance is not finite passes no gradient.  On a HIP device with float32 clouds the search is csrc/nearest.hip's
    (a sorted list of K keys per query in registers; no N x M tensor); otherwise a chunked torch expression."""
    x, y, x_lengths, y_lengths, single = _arguments(x, y, x_lengths, y_lengths)
    if not isinstance(K, int) or isinstance(K, bool) or not 1 <= K <= _native.KNN_MAX_K:
        raise ValueError("K must be an int in [1, %d], got %r" % (_native.KNN_MAX_K, K))
    if _on_hip_path(x):
        sqdist, idx = _Knn.apply(x, y, x_lengths, y_lengths, K)
    else:
        sqdist, idx = _knn_torch(x, y, K, x_lengths, y_lengths)
    out = (sqdist, idx, knn_gather(y, idx)) if return_nn else (sqdist, idx)
    return tuple(t[0] for t in out) if single else out


def _smallest_eigenvectors(c):
    """c [...,3,3] symmetric float64 -> (unit eigenvectors of the smallest eigenvalue [...,3], eigenvalues [...,3]
    ascending), in closed form with elementwise ops: the trigonometric eigenvalues, then the largest of the three cross
    products of the rows of c - lambda_0 I.  The zero vector where lambda_1 - lambda_0 <= 1e-12 lambda_2."""
    c00, c11, c22 = c[..., 0, 0], c[..., 1, 1], c[..., 2, 2]
    c01, c02, c12 = c[..., 0, 1], c[..., 0, 2], c[..., 1, 2]
    q = (c00 + c11 + c22) / 3.0
    off = c01 * c01 + c02 * c02 + c12 * c12
    p = (((c00 - q) ** 2 + (c11 - q) ** 2 + (c22 - q) ** 2 + 2.0 * off) / 6.0).sqrt()
    safe = p.clamp(min=1e-300)
    b00, b11, b22, b01, b02, b12 = ((c00 - q) / safe, (c11 - q) / safe, (c22 - q) / safe, c01 / safe, c02 / safe,
                                    c12 / safe)
    det = b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02)
    phi = torch.acos((det / 2.0).clamp(-1.0, 1.0)) / 3.0
    high = q + 2.0 * p * torch.cos(phi)
    low = q + 2.0 * p * torch.cos(phi + 2.0943951023931953)   # + 2 pi / 3
    mid = 3.0 * q - high - low
    rows = c - low[..., None, None] * torch.eye(3, dtype=c.dtype, device=c.device)
    crosses = torch.stack([torch.cross(rows[..., 0, :], rows[..., 1, :], dim=-1),
                           torch.cross(rows[..., 0, :], rows[..., 2, :], dim=-1),
                           torch.cross(rows[..., 1, :], rows[..., 2, :], dim=-1)], dim=-2)      # [...,3,3]
    norms = crosses.norm(dim=-1)
    which = norms.argmax(dim=-1)
    vector = torch.gather(crosses, -2, which[..., None, None].expand(*which.shape, 1, 3))[..., 0, :]
    length = torch.gather(norms, -1, which[..., None])
    usable = (mid - low > 1e-12 * high) & (length[..., 0] > 0)
    vector = torch.where(usable[..., None], vector / length.clamp(min=1e-300), torch.zeros_like(vector))
    return vector, torch.stack([low, mid, high], dim=-1)


def estimate_point_normals(points, K=16, lengths=None, orient_to=None):
    """points [B,N,3] (or [N,3]) -> unit normals [B,N,3] in the points' dtype: for every point the direction of least
    variance of its K nearest points of the same cloud, the point itself included (knn_points(points, points, K,
    lengths, lengths)): the covariance about the neighbourhood's mean in float64 and the eigenvector of its smallest
    eigenvalue in closed form (elementwise torch ops on the points' device, no solver).

    A neighbourhood with fewer than 3 valid points, a collinear one (lambda_1 - lambda_0 <= 1e-12 lambda_2) and a
    padded row get the zero vector.  Sign: with orient_to ([3] or [B,3], a sensor position) so that
    n . (orient_to - p) >= 0; otherwise the component of largest magnitude is positive (the lowest axis of equal
    magnitudes).  NOT differentiable: the scan is data, and the result carries no graph."""
    _cloud("points", points)
    single = points.dim() == 2
    p = points.detach().unsqueeze(0) if single else points.detach()
    B = p.shape[0]
    if single and torch.is_tensor(lengths) and lengths.dim() == 0:
        lengths = lengths.reshape(1)
    if orient_to is not None:
        if not torch.is_tensor(orient_to) or not orient_to.is_floating_point():
            raise TypeError("orient_to must be a floating-point tensor")
        if orient_to.shape not in ((3,), (B, 3)):
            raise ValueError("orient_to must have shape [3] or [%d, 3], got %s" % (B, list(orient_to.shape)))
        if orient_to.device != p.device:
            raise RuntimeError("orient_to must be on the points' device")
    with torch.no_grad():
        sqdist, idx = knn_points(p, p, K, lengths, lengths)
        valid = (idx >= 0) & torch.isfinite(sqdist)                               # [B,N,K]
        p64 = p.double()
        count = valid.sum(-1, keepdim=True).clamp(min=1).double()                 # [B,N,1]
        near = knn_gather(p64, idx)                                               # [B,N,K,3], zeros where invalid
        mean = near.sum(2) / count
        centred = torch.where(valid[..., None], near - mean[:, :, None, :], torch.zeros_like(near))
        covariance = (centred[..., :, None] * centred[..., None, :]).sum(2) / count[..., None]
        normals, _ = _smallest_eigenvectors(covariance)
        normals = torch.where((valid.sum(-1) >= 3)[..., None], normals, torch.zeros_like(normals))
        if orient_to is not None:
            towards = orient_to.detach().double().reshape(-1, 1, 3) - p64
            flip = (normals * towards).sum(-1, keepdim=True) < 0
        else:
            lead = torch.gather(normals, -1, normals.abs().argmax(dim=-1, keepdim=True))
            flip = lead < 0
        normals = torch.where(flip, -normals, normals).to(points.dtype)
    return normals[0] if single else normals


# ---- farthest-point sampling ------------------------------------------------------------------------------------------

def _farthest_torch(points, K, lengths, start_idx):
    """sample_farthest_points' indices and radii as a torch loop of K steps on the device and in the dtype of points
    [B,N,3], without a graph: the definition, step by step.  -> (idx [B,K] int32, radius [B,K])."""
    B, N, _ = points.shape
    dev, dtype = points.device, points.dtype
    with torch.no_grad():
        p = points.detach()
        n_valid = lengths.long() if lengths is not None else torch.full((B,), N, dtype=torch.int64, device=dev)
        position = torch.arange(N, device=dev)[None, :]
        valid = position < n_valid[:, None]
        finite = torch.isfinite(p).all(dim=-1)
        m = torch.where(finite, torch.full((B, N), float("inf"), dtype=dtype, device=dev),
                        torch.zeros((), dtype=dtype, device=dev))
        m = torch.where(valid, m, torch.full_like(m, -1.0))
        s = start_idx.long() if start_idx is not None else torch.zeros(B, dtype=torch.int64, device=dev)
        s = torch.minimum(s, n_valid - 1).clamp(min=0)
        r = torch.full((B,), float("inf"), dtype=dtype, device=dev)
        idx = torch.full((B, K), -1, dtype=torch.int64, device=dev)
        radius = torch.zeros(B, K, dtype=dtype, device=dev)
        for k in range(K):
            live = n_valid > k
            idx[:, k] = torch.where(live, s, torch.full_like(s, -1))
            radius[:, k] = torch.where(live, r, torch.zeros_like(r))
            if k + 1 == K:
                break
            diff = p - torch.gather(p, 1, s[:, None, None].expand(-1, 1, 3))
            dx, dy, dz = diff[..., 0], diff[..., 1], diff[..., 2]
            d = (dx * dx + dy * dy) + dz * dz
            m = torch.where(d < m, d, m)                       # a NaN distance changes nothing
            m.scatter_(1, s[:, None], -1.0)
            r = m.max(dim=1).values
            s = torch.where(m == r[:, None], position, torch.full_like(position, N)).min(dim=1).values   # the lowest
            s = s.clamp(max=N - 1)
    return idx.to(torch.int32), radius


def sample_farthest_points(points, K, lengths=None, start_idx=None, return_radius=False):
    """points [B,N,3] (or [N,3]: one cloud, results without the batch axis), K a Python int >= 1 -> (sampled [B,K,3],
    idx [B,K] int32[, radius [B,K] with return_radius]): K points of every cloud chosen greedily, each the farthest
    from those chosen before it.  The definition is part of the interface; length_b is lengths[b], or N:

      idx[b,0] = start_idx[b] clamped to [0, length_b) (0 without start_idx).  Every valid point carries a running
      distance m_i in the points' dtype, +inf at first.  After point s is selected, d_i = ((dx dx) + (dy dy)) + (dz dz)
      with dx = x_i - x_s, every operation rounded on its own in exactly this order; m_i becomes d_i if d_i < m_i (a NaN
      d_i changes nothing) and m_s becomes -1.  The next point is the one with the largest m_i, the lowest index among
      equals.

    The K indices of a cloud are pairwise distinct whenever K <= length_b (a duplicate of a selected point has
    m = 0 > -1 and is taken before anything repeats).  A point with a non-finite coordinate has m_i = 0 from the start
    and is never updated: it is selected only when nothing finite is farther than 0, and as a selected point it moves
    nobody.  Slots k >= length_b (an empty cloud, K > length_b) get idx -1 and sampled 0; padded coordinates
    influence nothing.  radius[b,k] is m of the selected point at the moment of its selection: +inf for slot 0,
    non-increasing from slot 1, 0 for empty slots; radius[b,K-1] is the squared distance within which the first K - 1
    samples cover the cloud.

    sampled = points at idx, a torch gather: differentiable in points, and a slot with idx -1 passes no gradient;
    the indices of a cloud are distinct, so the gradient is bitwise reproducible.  idx and radius are not
    differentiable.  lengths, start_idx: optional integer [B] tensors on the clouds' device, clamped on the device
    (nothing is read back).  On a HIP device with float32 clouds the selection is csrc/farthest.hip's (one launch that
    keeps the cloud in one workgroup's registers, or one launch per step for large clouds; bit-identical);
    otherwise a torch loop of K steps."""
    _cloud("points", points)
    if not isinstance(K, int) or isinstance(K, bool) or K < 1:
        raise ValueError("K must be an int >= 1, got %r" % (K,))
    single = points.dim() == 2
    p = points.unsqueeze(0) if single else points
    B, N, _ = p.shape
    if B < 1:
        raise ValueError("points must hold at least one cloud, got %s" % list(points.shape))
    if single:
        lengths = lengths.reshape(1) if torch.is_tensor(lengths) and lengths.dim() == 0 else lengths
        start_idx = start_idx.reshape(1) if torch.is_tensor(start_idx) and start_idx.dim() == 0 else start_idx
    lengths = _lengths("lengths", lengths, B, N, p)
    start_idx = _lengths("start_idx", start_idx, B, N - 1, p)
    if _on_hip_path(p):
        idx, radius = _native.farthest_forward(p.detach().contiguous(), K, lengths, start_idx)
    else:
        idx, radius = _farthest_torch(p, K, lengths, start_idx)
    sampled = knn_gather(p, idx[:, :, None])[:, :, 0]
    out = (sampled, idx, radius) if return_radius else (sampled, idx)
    return tuple(t[0] for t in out) if single else out


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


# ---- point to mesh: the nearest triangle ----------------------------------------------------------------------------

def _point_mesh_arguments(points, vertices, triangles, lengths):
    """-> (points [B,N,3], vertices [B,V,3], triangles [T,3] int64 on their device, lengths, whether the batch axis
    was missing)."""
    _cloud("points", points)
    v, tris, single = _mesh(vertices, triangles)
    if points.dim() != vertices.dim():
        raise ValueError("points and vertices must both have a batch axis or both lack it, got %s and %s"
                         % (list(points.shape), list(vertices.shape)))
    p = points.unsqueeze(0) if single else points
    if p.shape[0] != v.shape[0]:
        raise ValueError("points and vertices must have the same batch size, got %s and %s"
                         % (list(points.shape), list(vertices.shape)))
    if p.device != v.device:
        raise RuntimeError("points and vertices must be on the same device")
    if p.dtype != v.dtype:
        raise RuntimeError("points and vertices must have the same dtype, got %s and %s" % (p.dtype, v.dtype))
    if single and torch.is_tensor(lengths) and lengths.dim() == 0:
        lengths = lengths.reshape(1)
    return p, v, tris, _lengths("lengths", lengths, p.shape[0], p.shape[1], p), single


class _TriangleRecords:
    """What the search needs of every (image, triangle): a, e0 = b - a, e1 = c - a, e2 = c - b, the dot products and
    the reciprocals (0 where the denominator is not positive), each [B,T,...]; usable [T]."""

    def __init__(self, v, tris):
        V = v.shape[1]
        self.usable = ((tris >= 0) & (tris < V)).all(dim=1)
        safe = tris.clamp(0, V - 1)
        a, b, c = (v.index_select(1, safe[:, k]) for k in range(3))
        self.a, self.e0, self.e1, self.e2 = a, b - a, c - a, c - b
        self.d00, self.d01, self.d11 = (self.e0 * self.e0).sum(-1), (self.e0 * self.e1).sum(-1), (self.e1 * self.e1).sum(-1)
        d22 = (self.e2 * self.e2).sum(-1)
        det = self.d00 * self.d11 - self.d01 * self.d01
        inverse = lambda x: torch.where(x > 0, 1.0 / x, torch.zeros_like(x))
        self.idet, self.i00, self.i11, self.i22 = inverse(det), inverse(self.d00), inverse(self.d11), inverse(d22)

    def select(self, pick):
        """The records as seen by the queries: pick(t [B,T,...]) -> a tensor that broadcasts against [B,rows,...]."""
        out = object.__new__(_TriangleRecords)
        for name in ("a", "e0", "e1", "e2", "d00", "d01", "d11", "idet", "i00", "i11", "i22"):
            setattr(out, name, pick(getattr(self, name)))
        return out


def _triangle_candidates(p, r):
    """The four candidates of the definition for queries p [...,3] against records r that broadcast with them ->
    (squared distances [...,4] with +inf for a projection that is no candidate and for NaN, beta [...,4],
    gamma [...,4]) in the order projection, ab, bc, ca; every distance is |d - (beta e0 + gamma e1)|^2 with d = p - a
    (the segment bc from d - e0)."""
    d = p - r.a
    p0, p1 = (d * r.e0).sum(-1), (d * r.e1).sum(-1)
    sq = lambda x: (x * x).sum(-1)
    tab = (p0 * r.i00).clamp(0, 1)
    tca = (p1 * r.i11).clamp(0, 1)
    db = d - r.e0
    tbc = ((db * r.e2).sum(-1) * r.i22).clamp(0, 1)
    v = (p0 * r.d11 - p1 * r.d01) * r.idet
    w = (p1 * r.d00 - p0 * r.d01) * r.idet
    inside = (r.idet > 0) & (v >= 0) & (w >= 0) & (v + w <= 1)
    inf = torch.full_like(p0, float("inf"))
    dist = torch.stack([torch.where(inside, sq(d - v[..., None] * r.e0 - w[..., None] * r.e1), inf),
                        sq(d - tab[..., None] * r.e0), sq(db - tbc[..., None] * r.e2), sq(d - tca[..., None] * r.e1)], -1)
    dist = torch.where(dist == dist, dist, inf[..., None])   # a NaN never wins
    zero = torch.zeros_like(tab)
    return dist, torch.stack([v, tab, 1.0 - tbc, zero], -1), torch.stack([w, zero, tbc, tca], -1)


def _nearest_triangles_torch(points, v, tris, lengths):
    """nearest_triangles as a torch expression on the device and in the dtype of points [B,N,3] / v [B,V,3]: the face
    is searched chunk by chunk of queries without a graph; the distance to the closest point, its barycentrics held
    constant (the envelope theorem), is then an ordinary differentiable expression."""
    B, N, _ = points.shape
    T = tris.shape[0]
    dev = points.device
    n_valid = lengths.long() if lengths is not None else torch.full((B,), N, dtype=torch.int64, device=dev)
    with torch.no_grad():
        records = _TriangleRecords(v.detach(), tris)
        against_all = records.select(lambda t: t[:, None])                       # [B,1,T,...]
        rows = max(1, _CHUNK_BYTES // max(1, B * T * 12 * points.element_size()))
        faces, found = [], []
        for start in range(0, N, rows):
            dist, _, _ = _triangle_candidates(points.detach()[:, start:start + rows, None, :], against_all)
            best = dist.min(dim=-1).values.masked_fill(~records.usable[None, None, :], float("inf"))   # [B,rows,T]
            nearest = best.min(dim=2)                                             # the first of equal minima
            faces.append(nearest.indices)
            found.append(nearest.values < float("inf"))
        face = torch.cat(faces, dim=1)
        valid = torch.cat(found, dim=1) & (torch.arange(N, device=dev)[None, :] < n_valid[:, None])
        face = torch.where(valid, face, torch.zeros_like(face))
        chosen = records.select(lambda t: torch.gather(
            t, 1, face.reshape(B, N, *[1] * (t.dim() - 2)).expand(B, N, *t.shape[2:])))   # [B,N,...]
        dist, beta, gamma = _triangle_candidates(points.detach(), chosen)
        which = dist.min(dim=-1).indices[..., None]
        beta, gamma = torch.gather(beta, -1, which)[..., 0], torch.gather(gamma, -1, which)[..., 0]
        bary = torch.stack([(1.0 - (beta + gamma)).clamp(min=0), beta, gamma], -1)
        bary = torch.where(valid[..., None], bary, torch.zeros_like(bary))
    # differentiable: |d - (beta e0 + gamma e1)|^2 from the vertices of the chosen face
    corner = tris.clamp(0, v.shape[1] - 1)[face]                                 # [B,N,3]
    a, b, c = (torch.gather(v, 1, corner[..., k, None].expand(-1, -1, 3)) for k in range(3))
    residual = (points - a) - (bary[..., 1:2] * (b - a) + bary[..., 2:3] * (c - a))
    residual = torch.where(valid[..., None], residual, torch.zeros_like(residual))   # no result: value 0, gradient 0
    face = torch.where(valid, face, torch.full_like(face, -1))
    return (residual * residual).sum(-1), face.to(torch.int32), bary


class _NearestTriangles(torch.autograd.Function):
    """Both public functions on the HIP path.  reduce False: (sqdist [B,N], face [B,N], bary [B,N,3]); reduce True:
    the mean of sqdist over each image's valid queries [B]."""

    @staticmethod
    def forward(ctx, points, vertices, triangles, lengths, reduce):
        pd, vd = points.detach().contiguous(), vertices.detach().contiguous()
        sqdist, face, bary, total = _native.nearest_triangle_forward(pd, vd, triangles, lengths, want_sqdist=not reduce,
                                                                     want_total=reduce)
        ctx.reduce = reduce
        ctx.save_for_backward(pd, vd, triangles, lengths, face, bary)
        if reduce:
            return total
        ctx.mark_non_differentiable(face, bary)
        return sqdist, face, bary

    @staticmethod
    @once_differentiable
    def backward(ctx, grad, _face=None, _bary=None):
        points, vertices, triangles, lengths, face, bary = ctx.saved_tensors
        want_dp, want_dv = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        none = (None,) * 3
        if not (want_dp or want_dv):
            return (None, None) + none
        index = None
        if want_dv:   # the (query, corner) entries keyed by the vertex they name, -1 for rows without a face
            named = triangles[face.clamp(min=0).long()]                          # [B,N,3]
            named = torch.where(face[..., None] < 0, torch.full_like(named, -1), named)
            index = _native.nearest_inverted_index(named.reshape(face.shape[0], -1), vertices.shape[1])
        grad = grad.contiguous()
        dp, dv = _native.nearest_triangle_backward(
            points, vertices, triangles, lengths, face, bary, index, grad_points=None if ctx.reduce else grad,
            grad_images=grad if ctx.reduce else None, want_dpoints=want_dp, want_dvertices=want_dv)
        return (dp, dv) + none


def _device_triangles(tris, V):
    """int32 for the kernels; an index that int32 cannot hold is outside [0, V) either way."""
    return torch.where((tris >= 0) & (tris < V), tris, torch.full_like(tris, -1)).to(torch.int32).contiguous()


def nearest_triangles(points, vertices, triangles, lengths=None):
    """points [B,N,3], vertices [B,V,3] (or [N,3], [V,3]: one image, results without the batch axis), triangles [T,3]
    of any integer dtype (one topology for the batch) -> (sqdist [B,N], face [B,N] int32, bary [B,N,3]): for every
    point the squared Euclidean distance to the nearest CLOSED triangle (interior, edges and corners), the lowest
    face that attains it and the barycentrics of the closest point on that face (>= 0, adding up to 1).  A zero-area
    triangle counts as its edges or its point; a triangle with an index outside [0, V) is never chosen.

    sqdist is differentiable in points and vertices with the barycentrics held constant (the envelope theorem);
    face and bary are not differentiable.  lengths: an optional integer [B] tensor on the points' device for padded
    clouds, clamped to [0, N] on the device.  A padded row, and a point for which no triangle compared below +inf
    (no usable triangle, NaN coordinates), get sqdist 0, face -1, bary 0 and no gradient; padded coordinates
    influence nothing.  Every other face is a usable triangle's index."""
    p, v, tris, lengths, single = _point_mesh_arguments(points, vertices, triangles, lengths)
    if _on_hip_path(p):
        out = _NearestTriangles.apply(p, v, _device_triangles(tris, v.shape[1]), lengths, False)
    else:
        out = _nearest_triangles_torch(p, v, tris, lengths)
    return tuple(t[0] for t in out) if single else tuple(out)


def point_mesh_distance(points, vertices, triangles, lengths=None):
    """The mean over each image's valid points of nearest_triangles' sqdist -> [B] (a 0-dim tensor without the batch
    axis); 0 for an image without a valid point or a usable triangle.  The data term for fitting a mesh to a scan
    without the sampling noise of chamfer_distance against sampled points: the distance is to the surface itself.
    A fixed-order sum on a HIP device; differentiable in points and vertices, and a gradient that is not required is
    not computed."""
    p, v, tris, lengths, single = _point_mesh_arguments(points, vertices, triangles, lengths)
    if _on_hip_path(p):
        total = _NearestTriangles.apply(p, v, _device_triangles(tris, v.shape[1]), lengths, True)
    else:
        total = _mean_torch(_nearest_triangles_torch(p, v, tris, lengths)[0], lengths, None)
    return total[0] if single else total


# ---- mesh to point: the nearest point of every triangle -------------------------------------------------------------

def _triangle_nearest_points_torch(points, v, tris, lengths):
    """triangle_nearest_points as a torch expression on the device and in the dtype of points [B,N,3] / v [B,V,3]:
    the point is searched chunk by chunk of triangles without a graph; the distance from the triangle's closest point
    to it, the barycentrics held constant (the envelope theorem), is then an ordinary differentiable expression."""
    B, N, _ = points.shape
    T = tris.shape[0]
    dev = points.device
    n_valid = lengths.long() if lengths is not None else torch.full((B,), N, dtype=torch.int64, device=dev)
    with torch.no_grad():
        records = _TriangleRecords(v.detach(), tris)
        outside = torch.arange(N, device=dev)[None, None, :] >= n_valid[:, None, None]          # [B,1,N]
        cloud = points.detach()[:, None, :, :]                                                   # [B,1,N,3]
        rows = max(1, _CHUNK_BYTES // max(1, B * N * 12 * points.element_size()))
        chosen, found = [], []
        for start in range(0, T, rows):
            some = records.select(lambda t: t[:, start:start + rows, None])      # [B,rows,1,...]
            dist, _, _ = _triangle_candidates(cloud, some)
            best = dist.min(dim=-1).values.masked_fill(outside, float("inf"))    # [B,rows,N]
            nearest = best.min(dim=2)                                             # the first of equal minima
            chosen.append(nearest.indices)
            found.append(nearest.values < float("inf"))
        valid = torch.cat(found, dim=1) & records.usable[None, :]
        index = torch.where(valid, torch.cat(chosen, dim=1), torch.zeros((), dtype=torch.int64, device=dev))
        take = index[..., None].expand(-1, -1, 3)                                 # [B,T,3]
        dist, beta, gamma = _triangle_candidates(torch.gather(points.detach(), 1, take), records.select(lambda t: t))
        which = dist.min(dim=-1).indices[..., None]
        beta, gamma = torch.gather(beta, -1, which)[..., 0], torch.gather(gamma, -1, which)[..., 0]
        bary = torch.stack([(1.0 - (beta + gamma)).clamp(min=0), beta, gamma], -1)
        bary = torch.where(valid[..., None], bary, torch.zeros_like(bary))
    # differentiable: |d - (beta e0 + gamma e1)|^2 with d = p_index - a
    corner = tris.clamp(0, v.shape[1] - 1)
    a, b, c = (v.index_select(1, corner[:, k]) for k in range(3))
    residual = (torch.gather(points, 1, take) - a) - (bary[..., 1:2] * (b - a) + bary[..., 2:3] * (c - a))
    residual = torch.where(valid[..., None], residual, torch.zeros_like(residual))   # no result: value 0, gradient 0
    index = torch.where(valid, index, torch.full_like(index, -1))
    return (residual * residual).sum(-1), index.to(torch.int32), bary, records.usable.sum()


class _TriangleNearestPoints(torch.autograd.Function):
    """Both public functions on the HIP path.  reduce False: (sqdist [B,T], index [B,T], bary [B,T,3]); reduce True:
    the mean of sqdist over the usable triangles [B]."""

    @staticmethod
    def forward(ctx, points, vertices, triangles, lengths, reduce):
        pd, vd = points.detach().contiguous(), vertices.detach().contiguous()
        sqdist, index, bary, total, usable = _native.nearest_point_of_triangle_forward(
            pd, vd, triangles, lengths, want_sqdist=not reduce, want_total=reduce)
        ctx.reduce = reduce
        ctx.save_for_backward(pd, vd, triangles, lengths, index, bary, usable)
        if reduce:
            return total
        ctx.mark_non_differentiable(index, bary)
        return sqdist, index, bary

    @staticmethod
    @once_differentiable
    def backward(ctx, grad, _index=None, _bary=None):
        points, vertices, triangles, lengths, index, bary, usable = ctx.saved_tensors
        want_dp, want_dv = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        none = (None,) * 3
        if not (want_dp or want_dv):
            return (None, None) + none
        corner_index = point_index = None
        if want_dv:   # the (triangle, corner) entries keyed by the vertex they name, -1 for triangles without a point
            named = torch.where(index[..., None] < 0, torch.full_like(triangles, -1)[None], triangles[None])
            corner_index = _native.nearest_inverted_index(named.reshape(index.shape[0], -1), vertices.shape[1])
        if want_dp:   # the triangles keyed by the point they chose
            point_index = _native.nearest_inverted_index(index, points.shape[1])
        grad = grad.contiguous()
        dp, dv = _native.nearest_point_of_triangle_backward(
            points, vertices, triangles, lengths, index, bary, corner_index, point_index,
            grad_triangles=None if ctx.reduce else grad, grad_images=grad if ctx.reduce else None, usable=usable,
            want_dpoints=want_dp, want_dvertices=want_dv)
        return (dp, dv) + none


def triangle_nearest_points(points, vertices, triangles, lengths=None):
    """points [B,N,3], vertices [B,V,3] (or [N,3], [V,3]: one image, results without the batch axis), triangles [T,3]
    of any integer dtype (one topology for the batch) -> (sqdist [B,T], index [B,T] int32, bary [B,T,3]): for every
    triangle the squared Euclidean distance from the CLOSED triangle (interior, edges and corners) to the nearest
    valid point of its image, the lowest point index that attains it and the barycentrics of the triangle's closest
    point to that point (>= 0, adding up to 1).  The other direction of nearest_triangles, with the same arithmetic
    per (point, triangle) pair.  A zero-area triangle counts as its edges or its point.

    sqdist is differentiable in points and vertices with the barycentrics held constant (the envelope theorem);
    index and bary are not differentiable.  lengths: an optional integer [B] tensor on the points' device for padded
    clouds, clamped to [0, N] on the device; padded rows influence nothing.  A triangle with an index outside [0, V),
    and a triangle for which no point compared below +inf (lengths[b] = 0, NaN coordinates, a point at +-inf), get
    sqdist 0, index -1, bary 0 and no gradient.  Every other index lies in [0, lengths[b])."""
    p, v, tris, lengths, single = _point_mesh_arguments(points, vertices, triangles, lengths)
    if _on_hip_path(p):
        out = _TriangleNearestPoints.apply(p, v, _device_triangles(tris, v.shape[1]), lengths, False)
    else:
        out = _triangle_nearest_points_torch(p, v, tris, lengths)[:3]
    return tuple(t[0] for t in out) if single else tuple(out)


def mesh_point_distance(points, vertices, triangles, lengths=None):
    """The mean over the usable triangles (every index in [0, V): a property of the topology, the same count U for
    every image, formed on the device) of triangle_nearest_points' sqdist -> [B] (a 0-dim tensor without the batch
    axis); 0 where U = 0 or the image has no valid point; a usable triangle without a result adds 0 and counts.
    The mesh -> scan half of the exact data term: it keeps parts of the mesh that no scan point is near from being
    ignored, without sampling the surface.  A fixed-order sum on a HIP device; differentiable in points and vertices,
    and a gradient that is not required is not computed."""
    p, v, tris, lengths, single = _point_mesh_arguments(points, vertices, triangles, lengths)
    if _on_hip_path(p):
        total = _TriangleNearestPoints.apply(p, v, _device_triangles(tris, v.shape[1]), lengths, True)
    else:
        sqdist, _, _, usable = _triangle_nearest_points_torch(p, v, tris, lengths)
        total = sqdist.sum(1) / usable.clamp(min=1).to(sqdist.dtype)
    return total[0] if single else total


def point_mesh_face_distance(points, vertices, triangles, lengths=None):
    """point_mesh_distance(...) + mesh_point_distance(...): both directions of the exact distance between a scan and
    a mesh under PyTorch3D's name, each a mean of its own (over the valid points, over the usable triangles)."""
    return (point_mesh_distance(points, vertices, triangles, lengths)
            + mesh_point_distance(points, vertices, triangles, lengths))


# ---- inside or outside: the winding number and the signed distance ------------------------------------------------------

_WN_FRAC_BITS = 40          # csrc/wn_fixed.h: every term is rounded to a multiple of 2^-40 and summed in int64
_WN_MAX_TRIANGLES = 1 << 24


def _winding_number_torch(points, v, tris, lengths):
    """winding_number as a torch expression on the device and in the dtype of points [B,N,3] / v [B,V,3], chunked
    over the queries: the same definition as the kernels', the fixed-point sum included (the terms themselves are
    rounded by torch's own arithmetic, so the two routes agree within the rounding bound, not bit for bit)."""
    B, N, _ = points.shape
    V, T = v.shape[1], tris.shape[0]
    dev = points.device
    n_valid = lengths.long() if lengths is not None else torch.full((B,), N, dtype=torch.int64, device=dev)
    with torch.no_grad():
        points, v = points.detach(), v.detach()
        usable = (((tris >= 0) & (tris < V)).all(dim=1) & (tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2])
                  & (tris[:, 2] != tris[:, 0]))
        safe = tris.clamp(0, V - 1)
        va, vb, vc = (v.index_select(1, safe[:, k])[:, None] for k in range(3))          # [B,1,T,3]
        rows = max(1, _CHUNK_BYTES // max(1, B * T * 16 * points.element_size()))
        out = []
        for start in range(0, N, rows):
            p = points[:, start:start + rows, None, :]
            a, b, c = va - p, vb - p, vc - p
            la, lb, lc = (torch.sqrt((x * x).sum(-1)) for x in (a, b, c))
            num = (a * torch.cross(b, c, dim=-1)).sum(-1)
            den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
            finite = torch.isfinite(num) & torch.isfinite(den)
            turn = 2.0 * torch.atan2(num, den) / (4.0 * torch.pi)
            counted = usable[None, None, :] & finite
            fixed = torch.round(torch.where(counted, turn, torch.zeros_like(turn)).double() * 2.0 ** _WN_FRAC_BITS)
            w = fixed.to(torch.int64).sum(-1).to(points.dtype) * 2.0 ** -_WN_FRAC_BITS
            poisoned = (usable[None, None, :] & ~finite).any(-1)
            out.append(torch.where(poisoned, torch.full_like(w, float("nan")), w))
        w = torch.cat(out, dim=1)
        padded = torch.arange(N, device=dev)[None, :] >= n_valid[:, None]
        return torch.where(padded, torch.zeros_like(w), w)


def winding_number(points, vertices, triangles, lengths=None):
    """points [B,N,3], vertices [B,V,3] (or [N,3], [V,3]: one image, the result without the batch axis), triangles
    [T,3] of any integer dtype (one topology for the batch, at most 2^24 triangles) -> w [B,N]: the generalized
    winding number (Jacobson et al. 2013) of the mesh around every point, the sum of the signed solid angles of all
    triangles seen from the point over 4 pi.  With a = va - p, b = vb - p, c = vc - p per triangle:
        num = a . (b x c),   den = |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|,   t = 2 atan2(num, den) / (4 pi)
    For a closed mesh whose triangles are counter-clockwise seen from outside (shapes.cube) w is 1 inside and 0
    outside; for an open or folded mesh it degrades gracefully (0.96 at the centre of shapes.sphere, which is not
    watertight).  A triangle with an index outside [0, V) or with two equal indices is skipped.

    The sum is order-free: every term is rounded to the nearest multiple of 2^-40 and the rounded terms are added
    exactly as 64-bit integers, so on a HIP device (csrc/nearest.hip, k_wn_*) w is the same bit for bit whatever the
    order of the triangles, the launch shape or the batch an image sits in.  Host tensors and tensors that are not
    float32 take the torch expression of the same definition.

    lengths: an optional integer [B] tensor on the points' device for padded clouds; a padded row gets 0.  A point
    that meets a num or den that is not finite (a NaN or infinite point, a NaN vertex of a counted triangle) gets
    NaN; other points and other images are unaffected.

    NO GRADIENT: the result never requires grad.  For a closed mesh w is piecewise constant in the points and the
    vertices, so its gradient is zero almost everywhere and useless as a fitting signal; signed_distance is the
    differentiable companion."""
    p, v, tris, lengths, single = _point_mesh_arguments(points, vertices, triangles, lengths)
    if tris.shape[0] > _WN_MAX_TRIANGLES:
        raise ValueError("winding_number takes at most 2^24 triangles (the fixed-point sum's range), got %d"
                         % tris.shape[0])
    if _on_hip_path(p):
        w = _native.winding_number_forward(p.detach(), v.detach(), _device_triangles(tris, v.shape[1]), lengths)
    else:
        w = _winding_number_torch(p, v, tris, lengths)
    return w[0] if single else w


def inside_mesh(points, vertices, triangles, lengths=None, threshold=0.5):
    """winding_number(...) >= threshold -> bool [B,N]: which points the mesh encloses.  NaN and padded rows give
    False."""
    return winding_number(points, vertices, triangles, lengths) >= threshold


def signed_distance(points, vertices, triangles, lengths=None, threshold=0.5):
    """The distance of every point to the mesh's surface with the sign of inside_mesh -> [B,N]: s sqrt(sqdist) with
    sqdist from nearest_triangles and s = -1 where winding_number >= threshold, +1 elsewhere (NaN winding numbers
    included).  Differentiable in points and vertices through nearest_triangles' backward; s is a constant in the
    gradient, and the gradient is 0, not NaN, where the distance is 0.  A padded row, and a point without a nearest
    triangle, get 0."""
    sqdist = nearest_triangles(points, vertices, triangles, lengths)[0]
    inside = inside_mesh(points, vertices, triangles, lengths, threshold)
    nonzero = sqdist > 0   # the _safe_norm pattern of regularizers.py: sqrt never sees the 0 whose slope is infinite
    distance = torch.where(nonzero, torch.sqrt(torch.where(nonzero, sqdist, torch.ones_like(sqdist))),
                           torch.zeros_like(sqdist))
    return torch.where(inside, -distance, distance)


# ---- ray casting: where a ray first meets the mesh ------------------------------------------------------------------------

_RAY_MAX_TRIANGLES = 1 << 24   # the winding number's size limits (include/mesh_raster.h)


def _pick(x, k):
    """x [...,3], k [...] int64 -> x[..., k] [...]."""
    return torch.gather(x, -1, k[..., None].expand(*x.shape[:-1], 1))[..., 0]


def _cast_rays_torch(o, d, v, tris, lengths, t_min, t_max):
    """cast_rays as a torch expression on the device and in the dtype of o, d [B,N,3] / v [B,V,3], chunked over the
    rays, without a graph: the definition of include/mesh_raster.h operation by operation.  The fused multiply-add of
    the shear is formed in float64 and rounded back (the product is exact there), the edge functions are two rounded
    products and a rounded difference in the tensors' dtype and are recomputed in float64 where one is exactly 0.  The
    shear is applied per VERTEX and gathered per triangle, so two triangles see the same numbers at a shared corner."""
    B, N, _ = o.shape
    V, T = v.shape[1], tris.shape[0]
    dev, dtype = o.device, o.dtype
    n_valid = lengths.long() if lengths is not None else torch.full((B,), N, dtype=torch.int64, device=dev)
    with torch.no_grad():
        o, d, v = o.detach(), d.detach(), v.detach()
        safe = tris.clamp(0, V - 1)
        finite = torch.isfinite(v).all(-1)                                                # [B,V]
        usable = (((tris >= 0) & (tris < V)).all(dim=1) & (tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2])
                  & (tris[:, 2] != tris[:, 0]))[None] & finite[:, safe[:, 0]] & finite[:, safe[:, 1]] & finite[:, safe[:, 2]]
        lo, hi = torch.tensor(t_min, dtype=dtype, device=dev), torch.tensor(t_max, dtype=dtype, device=dev)
        inf = torch.tensor(float("inf"), dtype=dtype, device=dev)
        rows = max(1, _CHUNK_BYTES // max(1, B * max(T, V) * 24 * 8))
        ts, faces, barys = [], [], []
        for start in range(0, N, rows):
            oc, dc = o[:, start:start + rows], d[:, start:start + rows]
            R = oc.shape[1]
            size = dc.abs().max(-1).values
            live = (torch.isfinite(oc).all(-1) & torch.isfinite(dc).all(-1) & (size > 0)
                    & (torch.arange(start, start + R, device=dev)[None, :] < n_valid[:, None]))
            oc = torch.where(live[..., None], oc, torch.zeros_like(oc))
            dc = torch.where(live[..., None], dc, torch.ones_like(dc))
            kz = (dc.abs() == dc.abs().max(-1, keepdim=True).values).to(torch.uint8).argmax(-1)   # the first that attains
            kx, ky = (kz + 1) % 3, (kz + 2) % 3
            dz = _pick(dc, kz)
            kx, ky = torch.where(dz < 0, ky, kx), torch.where(dz < 0, kx, ky)
            sx, sy, sz = _pick(dc, kx) / dz, _pick(dc, ky) / dz, 1.0 / dz
            p = v[:, None] - oc[:, :, None]                                              # [B,R,V,3]
            wide = lambda k: _pick(p, k[..., None].expand(B, R, V)).double()
            pk = wide(kz)
            px = (wide(kx) - sx.double()[..., None] * pk).to(dtype)                       # fma(-Sx, p[kz], p[kx])
            py = (wide(ky) - sy.double()[..., None] * pk).to(dtype)
            pz = sz[..., None] * pk.to(dtype)
            ax, bx, cx = (px[:, :, safe[:, k]] for k in range(3))                         # [B,R,T]
            ay, by, cy = (py[:, :, safe[:, k]] for k in range(3))
            az, bz, cz = (pz[:, :, safe[:, k]] for k in range(3))
            u, vv, w = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
            zero = (u == 0) | (vv == 0) | (w == 0)
            u64, v64, w64 = u.double(), vv.double(), w.double()
            if bool(zero.any()):
                ax, ay, bx, by, cx, cy = (x.double() for x in (ax, ay, bx, by, cx, cy))
                u64 = torch.where(zero, cx * by - cy * bx, u64)
                v64 = torch.where(zero, ax * cy - ay * cx, v64)
                w64 = torch.where(zero, bx * ay - by * ax, w64)
            mixed = ((u64 < 0) | (v64 < 0) | (w64 < 0)) & ((u64 > 0) | (v64 > 0) | (w64 > 0))
            u, vv, w = u64.to(dtype), v64.to(dtype), w64.to(dtype)
            det = (u + vv) + w
            t = ((u * az + vv * bz) + w * cz) / det
            accept = usable[:, None, :] & live[..., None] & ~mixed & (det != 0) & (t >= lo) & (t <= hi)
            t = torch.where(accept, torch.where(t == 0, torch.zeros_like(t), t), inf)      # -0 is stored as +0
            first = t.min(dim=2)                                                          # the first of equal minima
            hit, index = first.values < inf, first.indices
            at = lambda x: torch.gather(x, 2, index[..., None])[..., 0]
            bary = torch.stack([at(u), at(vv), at(w)], -1) / torch.where(hit, at(det), torch.ones_like(first.values))[..., None]
            ts.append(first.values)
            faces.append(torch.where(hit, index, torch.full_like(index, -1)))
            barys.append(torch.where(hit[..., None], bary, torch.zeros_like(bary)))
        return torch.cat(ts, dim=1), torch.cat(faces, dim=1).to(torch.int32), torch.cat(barys, dim=1)


def _ray_gradients_torch(d, v, tris, t, face, bary, grad, want=(True, True, True)):
    """The analytic gradients of sum_i grad_i t_i with the face held fixed -> (dorigins, ddirections, dvertices), None
    for what is not wanted: with n = (b - a) x (c - a) and g = n / (n . d), dt/do = -g, dt/dd = -t g, dt/dv_k =
    bary_k g; 0 for a ray without a hit, with n . d == 0 or with a g that is not finite."""
    V = v.shape[1]
    hit = face >= 0
    corner = tris.long().clamp(0, V - 1)[face.clamp(min=0).long()]                        # [B,N,3]
    a, b, c = (torch.gather(v, 1, corner[..., k, None].expand(-1, -1, 3)) for k in range(3))
    n = torch.cross(b - a, c - a, dim=-1)
    s = (n * d).sum(-1)
    ok = hit & (s != 0)
    g = n / torch.where(ok, s, torch.ones_like(s))[..., None]
    ok = ok & torch.isfinite(g).all(-1)
    g = torch.where(ok[..., None], g, torch.zeros_like(g)) * torch.where(ok, grad, torch.zeros_like(grad))[..., None]
    dorigins = -g if want[0] else None
    ddirections = -g * torch.where(ok, t, torch.zeros_like(t))[..., None] if want[1] else None
    dvertices = None
    if want[2]:
        dvertices = torch.zeros_like(v)
        for k in range(3):
            dvertices.scatter_add_(1, corner[..., k, None].expand(-1, -1, 3), bary[..., k, None] * g)
    return dorigins, ddirections, dvertices


class _CastRays(torch.autograd.Function):
    """cast_rays on both routes: (t [B,N], face [B,N], bary [B,N,3]); the backward holds the face fixed and computes
    only the gradients that are required."""

    @staticmethod
    def forward(ctx, origins, directions, vertices, triangles, lengths, t_min, t_max):
        od, dd, vd = origins.detach().contiguous(), directions.detach().contiguous(), vertices.detach().contiguous()
        ctx.hip = _on_hip_path(od)
        if ctx.hip:
            triangles = _device_triangles(triangles, vd.shape[1])
            t, face, bary = _native.cast_rays_forward(od, dd, vd, triangles, lengths, t_min, t_max)
        else:
            t, face, bary = _cast_rays_torch(od, dd, vd, triangles, lengths, t_min, t_max)
        ctx.save_for_backward(dd, vd, triangles, lengths, t, face, bary)
        ctx.mark_non_differentiable(face, bary)
        return t, face, bary

    @staticmethod
    @once_differentiable
    def backward(ctx, grad, _face=None, _bary=None):
        directions, vertices, triangles, lengths, t, face, bary = ctx.saved_tensors
        want = tuple(ctx.needs_input_grad[:3])
        none = (None,) * 4
        if not any(want):
            return (None, None, None) + none
        grad = grad.contiguous()
        if not ctx.hip:
            return _ray_gradients_torch(directions, vertices, triangles, t, face, bary, grad, want) + none
        index = None
        if want[2]:   # the (ray, corner) entries keyed by the vertex they name, -1 for rays without a hit
            named = triangles[face.clamp(min=0).long()]                                  # [B,N,3]
            named = torch.where(face[..., None] < 0, torch.full_like(named, -1), named)
            index = _native.nearest_inverted_index(named.reshape(face.shape[0], -1), vertices.shape[1])
        return _native.cast_rays_backward(directions, vertices, triangles, lengths, t, face, bary, grad, index,
                                          want_dorigins=want[0], want_ddirections=want[1], want_dvertices=want[2]) + none


def cast_rays(origins, directions, vertices, triangles, lengths=None, t_min=0.0, t_max=float("inf")):
    """origins, directions [B,N,3], vertices [B,V,3] (or [N,3], [V,3]: one image, results without the batch axis),
    triangles [T,3] of any integer dtype (one topology for the batch, at most 2^24 triangles) -> (t [B,N], face [B,N]
    int32, bary [B,N,3]): where every ray first meets the mesh.  Directions are NOT normalised: t is in units of |d|
    and the hit point is origins + t[..., None] * directions; bary are the hit point's barycentrics on the face.

    The test is the watertight one of Woop, Benthin and Wald (2013), stated operation by operation in
    include/mesh_raster.h and INTEGRATION.md ("Point-cloud losses"): a ray aimed at a shared edge or a vertex of a
    closed mesh cannot slip between two triangles.  The first hit is the accepted triangle with the least t in
    [t_min, t_max] (Python floats, 0 <= t_min <= t_max, rounded to the tensors' dtype); equal t goes to the lowest
    face.  There is no back-face culling.  A triangle with an index outside [0, V), two equal indices or a corner that
    is not finite is never hit.

    A ray without a hit -- a padded row (lengths: an optional integer [B] tensor on the rays' device), a non-finite
    origin or direction, a zero direction, nothing in [t_min, t_max] -- gets t = +inf, face = -1, bary = 0 and no
    gradient.  t is differentiable in origins, directions and vertices with the face held fixed: with n = (b - a) x
    (c - a) and g = n / (n . d), dt/do = -g, dt/dd = -t g, dt/dv_k = bary_k g, and 0 (never NaN) where n . d is 0 or g
    is not finite; a gradient that is not required is not computed.  face and bary are not differentiable.

    On a HIP device with float32 tensors the search runs in csrc/nearest.hip (k_ray_*): t, face and bary of a ray are
    the same bit for bit whatever the batch it sits in.  Host tensors and tensors that are not float32 take the torch
    expression of the same definition."""
    p, v, tris, lengths, single = _point_mesh_arguments(origins, vertices, triangles, lengths)
    _cloud("directions", directions)
    if directions.shape != origins.shape:
        raise ValueError("origins and directions must have the same shape, got %s and %s"
                         % (list(origins.shape), list(directions.shape)))
    if directions.device != p.device:
        raise RuntimeError("origins and directions must be on the same device")
    if directions.dtype != p.dtype:
        raise RuntimeError("origins and directions must have the same dtype, got %s and %s" % (p.dtype, directions.dtype))
    if isinstance(t_min, bool) or isinstance(t_max, bool) or not all(isinstance(x, (int, float)) for x in (t_min, t_max)):
        raise ValueError("t_min and t_max must be Python floats, got %r and %r" % (t_min, t_max))
    if not 0.0 <= t_min <= t_max:
        raise ValueError("0 <= t_min <= t_max is required, got %r and %r" % (t_min, t_max))
    if tris.shape[0] > _RAY_MAX_TRIANGLES:
        raise ValueError("cast_rays takes at most 2^24 triangles, got %d" % tris.shape[0])
    d = directions.unsqueeze(0) if single else directions
    out = _CastRays.apply(p, d, v, tris, lengths, float(t_min), float(t_max))
    return tuple(x[0] for x in out) if single else tuple(out)


def rays_occluded(origins, directions, vertices, triangles, lengths=None, t_min=0.0, t_max=float("inf")):
    """cast_rays(...)[1] >= 0 -> bool [B,N]: whether the mesh meets the ray within [t_min, t_max].  With the direction
    q - p and t_max = 1 it is the line of sight from p to q."""
    return cast_rays(origins, directions, vertices, triangles, lengths, t_min, t_max)[1] >= 0


# ---- registration: the similarity transform between matched points, and ICP ---------------------------------------------

SimilarityTransform = collections.namedtuple("SimilarityTransform", ["R", "T", "s"])
ICPSolution = collections.namedtuple("ICPSolution", ["converged", "rmse", "Xt", "RTs", "iterations"])


def _alignment_torch(x, y, weights, lengths, estimate_scale, allow_reflection):
    """corresponding_points_alignment's definition on the device and in the dtype of x [B,N,3] / y [B,N,3], with
    torch.linalg.svd and ordinary autograd -> (R [B,3,3], T [B,3], s [B], mean squared residual [B])."""
    B, N, _ = x.shape
    w = weights if weights is not None else x.new_ones(B, N)
    if lengths is not None:
        valid = torch.arange(N, device=x.device)[None, :] < lengths[:, None]
        w = torch.where(valid, w, torch.zeros_like(w))
        x = torch.where(valid[..., None], x, torch.zeros_like(x))   # padded coordinates influence nothing, NaN included
        y = torch.where(valid[..., None], y, torch.zeros_like(y))
    W = w.sum(1)
    empty = ~(W > 0) & (W == W)   # (a NaN weight is not "empty": it makes the image NaN)
    iw = 1.0 / torch.where(empty, torch.ones_like(W), W)
    # the means about a reference point, the first row of positive weight (as the kernels take it per chunk): coincident
    # points then have a variance of exactly 0, and a row that is not counted never enters.  The weight multiplies
    # first everywhere, so that a far-away row of weight 0 contributes an exact 0 and never an overflowed product.
    first = (w.detach() > 0).to(torch.int8).argmax(1)[:, None, None].expand(B, 1, 3)
    px, py = torch.gather(x.detach(), 1, first), torch.gather(y.detach(), 1, first)
    xm = px[:, 0] + (w[..., None] * (x - px)).sum(1) * iw[:, None]
    ym = py[:, 0] + (w[..., None] * (y - py)).sum(1) * iw[:, None]
    xc, yc = x - xm[:, None], y - ym[:, None]
    wxc = w[..., None] * xc
    C = torch.einsum("bni,bnj->bij", wxc, yc) * iw[:, None, None]
    var_x = (wxc * xc).sum(-1).sum(1) * iw
    eye = torch.eye(3, dtype=x.dtype, device=x.device).expand(B, 3, 3)
    # a non-finite coordinate or weight: the image's outputs are NaN (and torch.linalg.svd never sees it)
    poisoned = ~torch.isfinite(C.detach()).all(-1).all(-1) | ~torch.isfinite(var_x.detach())
    degenerate = empty | (C.detach().abs().amax(dim=(1, 2)) == 0)    # W = 0, or C = 0: R = I
    U, S, Vh = torch.linalg.svd(torch.where((degenerate | poisoned)[:, None, None], eye, C))
    if allow_reflection:
        last = torch.ones_like(W)
    else:
        last = torch.where(torch.det(U.detach() @ Vh.detach()) < 0, -torch.ones_like(W), torch.ones_like(W))
    E = torch.stack([torch.ones_like(last), torch.ones_like(last), last], dim=-1)
    R = torch.where(degenerate[:, None, None], eye, (U * E[:, None, :]) @ Vh)
    trace = torch.where(degenerate, torch.zeros_like(W), (S * E).sum(-1))
    if estimate_scale:
        usable = var_x > 0
        s = torch.where(usable, trace / torch.where(usable, var_x, torch.ones_like(var_x)), torch.ones_like(W))
    else:
        s = torch.ones_like(W)
    T = torch.where(empty[:, None], torch.zeros_like(ym), ym - s[:, None] * torch.einsum("bi,bij->bj", xm, R))
    residual = s[:, None, None] * (xc @ R) - yc
    residual = torch.where((w == 0)[..., None], torch.zeros_like(residual), residual)   # (its square may overflow)
    mse = (w * (residual * residual).sum(-1)).sum(1) * iw
    nan = torch.full_like(W, float("nan"))
    R = torch.where(poisoned[:, None, None], nan[:, None, None], R)
    T = torch.where(poisoned[:, None], nan[:, None], T)
    s = torch.where(poisoned, nan, s)
    return R, T, s, mse


def _alignment_arguments(x, y, weights, lengths):
    _cloud("x", x)
    _cloud("y", y)
    if x.shape != y.shape:
        raise ValueError("x and y must have the same shape (they are matched row by row), got %s and %s"
                         % (list(x.shape), list(y.shape)))
    if x.device != y.device:
        raise RuntimeError("x and y must be on the same device")
    if x.dtype != y.dtype:
        raise RuntimeError("x and y must have the same dtype, got %s and %s" % (x.dtype, y.dtype))
    single = x.dim() == 2
    if single:
        x, y = x.unsqueeze(0), y.unsqueeze(0)
        weights = weights.unsqueeze(0) if torch.is_tensor(weights) and weights.dim() == 1 else weights
        lengths = lengths.reshape(1) if torch.is_tensor(lengths) and lengths.dim() == 0 else lengths
    B, N, _ = x.shape
    if B < 1:
        raise ValueError("x must hold at least one image, got %s" % list(x.shape))
    if weights is not None:
        if not torch.is_tensor(weights) or not weights.is_floating_point():
            raise TypeError("weights must be a floating-point tensor")
        if weights.shape != (B, N):
            raise ValueError("weights must have shape [%d, %d], got %s" % (B, N, list(weights.shape)))
        if weights.device != x.device:
            raise RuntimeError("weights must be on the clouds' device")
        if weights.dtype != x.dtype:
            raise RuntimeError("weights must have the clouds' dtype, got %s and %s" % (weights.dtype, x.dtype))
    return x, y, weights, _lengths("lengths", lengths, B, N, x), single


def corresponding_points_alignment(x, y, weights=None, lengths=None, estimate_scale=False, allow_reflection=False):
    """x, y [B,N,3] (or [N,3]: one image, results without the batch axis), matched row by row -> SimilarityTransform(
    R [B,3,3], T [B,3], s [B]) with s * x @ R + T ~ y (PyTorch3D's name and row-vector convention): the weighted
    least-squares similarity (Umeyama).  weights [B,N] >= 0 optional; lengths [B] as everywhere in this module
    (clamped on the device, padded rows influence nothing).  The definition is part of the interface:

      W = sum w; xm, ym the weighted means; C = sum w (x - xm)(y - ym)^T / W = U S V^T;
      E = diag(1, 1, det(U V^T)), or I with allow_reflection; R = U E V^T;
      s = tr(S E) / (sum w |x - xm|^2 / W) with estimate_scale, else 1; T = ym - s xm R.

    W = 0 (an empty image, all weights 0) gives R = I, T = 0, s = 1; zero variance of x gives s = 1; C = 0 gives
    R = I; a rank-deficient C (collinear or coincident points) gives a finite orthonormal R of the required
    determinant whose residual is the minimum -- which of the equal minimisers is not specified.  A non-finite
    coordinate in a valid row makes that image's outputs non-finite and touches no other image.

    float32 device tensors none of which requires a gradient go through csrc/align.hip (float64 moments in a fixed
    order, one Jacobi SVD per image in float64, rounded once; bitwise reproducible, capturable).  Inputs that require
    a gradient, host tensors and other dtypes take the torch spelling: the definition above in the inputs' dtype with
    torch.linalg.svd and ordinary autograd."""
    x, y, weights, lengths, single = _alignment_arguments(x, y, weights, lengths)
    needs_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, y, weights))
    if _on_hip_path(x) and not needs_grad:
        R, T, s, _ = _native.align_solve(x.detach(), y.detach(), weights.detach() if weights is not None else None,
                                         lengths, estimate_scale=bool(estimate_scale),
                                         allow_reflection=bool(allow_reflection))
    else:
        R, T, s, _ = _alignment_torch(x, y, weights, lengths, bool(estimate_scale), bool(allow_reflection))
    return SimilarityTransform(R[0], T[0], s[0]) if single else SimilarityTransform(R, T, s)


def _closest_points_torch(xt, v, tris, lengths):
    """-> (sqdist [B,N], kept [B,N] bool, the closest point of the nearest triangle [B,N,3])."""
    sqdist, face, bary = _nearest_triangles_torch(xt, v, tris, lengths)
    corner = tris.clamp(0, v.shape[1] - 1)[face.long().clamp(min=0)]                      # [B,N,3]
    corners = torch.stack([torch.gather(v, 1, corner[..., k, None].expand(-1, -1, 3)) for k in range(3)], dim=2)
    return sqdist, face >= 0, (bary[..., None] * corners).sum(2)


def _icp_torch(x, target, x_lengths, y_lengths, init, max_iterations, relative_rmse_thr, estimate_scale,
               allow_reflection, max_sqdist, check_every):
    """iterative_closest_point's rounds in torch ops on the device and in the dtype of x, image by image frozen as the
    kernels freeze them (the flags live on the device here too)."""
    B, N, _ = x.shape
    dev, dtype = x.device, x.dtype
    if init is None:
        R, T, s = torch.eye(3, dtype=dtype, device=dev).repeat(B, 1, 1), x.new_zeros(B, 3), x.new_ones(B)
    else:
        R, T, s = (t.clone() for t in init)
    n_valid = x_lengths.long() if x_lengths is not None else torch.full((B,), N, dtype=torch.int64, device=dev)
    valid = torch.arange(N, device=dev)[None, :] < n_valid[:, None]
    x = torch.where(valid[..., None], x, torch.zeros_like(x))
    apply = lambda: torch.where(valid[..., None], s[:, None, None] * (x @ R) + T[:, None, :], torch.zeros_like(x))
    rmse, prev = x.new_zeros(B), x.new_zeros(B)
    converged = torch.zeros(B, dtype=torch.bool, device=dev)
    iterations = torch.zeros(B, dtype=torch.int32, device=dev)
    for round_ in range(max_iterations):
        xt = apply()
        if target[0] == "cloud":
            sqdist, idx = _nearest_torch(xt, target[1], x_lengths, y_lengths)
            kept = idx >= 0
            match = torch.gather(target[1], 1, idx.long().clamp(min=0)[..., None].expand(-1, -1, 3))
        else:
            sqdist, kept, match = _closest_points_torch(xt, target[1], target[2], x_lengths)
        if max_sqdist is not None:
            kept = kept & (sqdist <= max_sqdist)
        kept = kept & valid
        match = torch.where(kept[..., None], match, torch.zeros_like(match))
        nR, nT, ns, mse = _alignment_torch(torch.where(kept[..., None], x, torch.zeros_like(x)), match, kept.to(dtype),
                                           None, estimate_scale, allow_reflection)
        root = mse.clamp(min=0).sqrt()
        nothing = ~kept.any(dim=1)
        live = ~converged
        change = live & ~nothing
        R = torch.where(change[:, None, None], nR, R)
        T = torch.where(change[:, None], nT, T)
        s = torch.where(change, ns, s)
        rmse = torch.where(live, torch.where(nothing, torch.zeros_like(root), root), rmse)
        iterations = iterations + live.to(torch.int32)
        done = nothing | (root == 0) | ((iterations >= 2) & ((prev - root) / prev <= relative_rmse_thr))
        prev = torch.where(live, rmse, prev)
        converged = converged | (live & done)
        if check_every and (round_ + 1) % check_every == 0 and round_ + 1 < max_iterations and bool(converged.all()):
            break
    return converged, rmse, apply(), R, T, s, iterations


def iterative_closest_point(x, y, x_lengths=None, y_lengths=None, init_transform=None, max_iterations=100,
                            relative_rmse_thr=1e-6, estimate_scale=False, allow_reflection=False,
                            max_correspondence_distance=None, check_every=10):
    """Registers the cloud x [B,N,3] (or [N,3]: one image, results without the batch axis) to y: a cloud [B,M,3], or a
    mesh (vertices [B,V,3], triangles [T,3] integer, one topology for the batch) -> ICPSolution(converged [B] bool,
    rmse [B], Xt [B,N,3], RTs SimilarityTransform(R, T, s), iterations [B] int32), PyTorch3D's name and row-vector
    convention s * x @ R + T ~ y.  For a mesh the match of a point is its closest point on the nearest triangle
    (nearest_triangles' sum of bary * corner): the surface itself, without the sampling noise at which ICP against
    sampled points stalls.

    One round, per image: Xt = s x R + T; search Xt -> y; keep the matches with sqdist <= max_correspondence_distance^2
    (all of them without one); solve corresponding_points_alignment of the ORIGINAL x to the kept matches, so rounding
    never accumulates over rounds; rmse = the root of the mean squared residual of the new transform on those matches.
    The image has converged when rmse == 0 or, from its second round on, (prev_rmse - rmse) / prev_rmse <=
    relative_rmse_thr; an image with no kept match converges at once with its transform unchanged and rmse 0.

    Convergence is per image and on the device: once an image has converged, its R, T, s, rmse and iterations never
    change again, bit for bit, whatever the other images of the batch do -- a batched call equals the single-image
    calls.  The host reads the flags back only every check_every rounds, to stop early; check_every=0 never reads
    anything back and runs exactly max_iterations rounds, which is the form torch.cuda.graph can capture.  Xt is the
    original cloud under the returned transform, 0 in padded rows.  init_transform: a SimilarityTransform (or any
    (R, T, s)) to start from, the identity without one.  x_lengths, y_lengths as in nearest_points (a mesh target
    takes no y_lengths).  PyTorch3D's t_history and verbose are not offered.

    The outputs are NOT differentiable and carry no graph.  float32 device tensors run csrc/align.hip around the
    module's own searches (apply, search, moments, solve: a fixed chain of launches per round, every buffer allocated
    before the first round, bitwise reproducible); host tensors and other dtypes take the same rounds in torch ops."""
    _cloud("x", x)
    for name, value in (("max_iterations", max_iterations), ("check_every", check_every)):
        if not isinstance(value, int) or isinstance(value, bool) or value < 0:
            raise ValueError("%s must be an int >= 0, got %r" % (name, value))
    if max_correspondence_distance is not None and not float(max_correspondence_distance) >= 0:
        raise ValueError("max_correspondence_distance must be >= 0, got %r" % (max_correspondence_distance,))
    is_mesh = isinstance(y, (tuple, list))
    with torch.no_grad():
        if is_mesh:
            if len(y) != 2:
                raise ValueError("a mesh target is (vertices, triangles), got %d entries" % len(y))
            if y_lengths is not None:
                raise ValueError("a mesh target takes no y_lengths")
            p, v, tris, x_lengths, single = _point_mesh_arguments(x.detach(), y[0].detach() if torch.is_tensor(y[0])
                                                                  else y[0], y[1], x_lengths)
            target = ("mesh", v, tris)
        else:
            p, cloud, x_lengths, y_lengths, single = _arguments(x.detach(), y.detach() if torch.is_tensor(y) else y,
                                                                x_lengths, y_lengths)
            target = ("cloud", cloud)
        B = p.shape[0]
        init = None
        if init_transform is not None:
            if len(init_transform) != 3 or not all(torch.is_tensor(t) for t in init_transform):
                raise ValueError("init_transform must be (R, T, s) tensors")
            R0, T0, s0 = (t.detach() for t in init_transform)
            if single and R0.dim() == 2:
                R0, T0, s0 = R0.unsqueeze(0), T0.unsqueeze(0), s0.reshape(1)
            if R0.shape != (B, 3, 3) or T0.shape != (B, 3) or s0.shape != (B,):
                raise ValueError("init_transform must hold R [%d, 3, 3], T [%d, 3] and s [%d], got %s, %s and %s"
                                 % (B, B, B, list(R0.shape), list(T0.shape), list(s0.shape)))
            if any(t.device != p.device for t in (R0, T0, s0)):
                raise RuntimeError("init_transform must be on the clouds' device")
            if any(t.dtype != p.dtype for t in (R0, T0, s0)):
                raise RuntimeError("init_transform must have the clouds' dtype")
            init = (R0, T0, s0)
        cut = float(max_correspondence_distance) ** 2 if max_correspondence_distance is not None else None
        if _on_hip_path(p):
            on_device = dict(y=target[1]) if not is_mesh else dict(mesh=(target[1], _device_triangles(tris, v.shape[1])))
            converged, rmse, xt, R, T, s, iterations = _native.icp(
                p, x_lengths=x_lengths, y_lengths=y_lengths, init=init, max_iterations=max_iterations,
                relative_rmse_thr=float(relative_rmse_thr), estimate_scale=bool(estimate_scale),
                allow_reflection=bool(allow_reflection), max_sqdist=cut, check_every=check_every, **on_device)
            converged = converged != 0
        else:
            converged, rmse, xt, R, T, s, iterations = _icp_torch(
                p, target, x_lengths, y_lengths, init, max_iterations, float(relative_rmse_thr), bool(estimate_scale),
                bool(allow_reflection), cut, check_every)
    if single:
        return ICPSolution(converged[0], rmse[0], xt[0], SimilarityTransform(R[0], T[0], s[0]), iterations[0])
    return ICPSolution(converged, rmse, xt, SimilarityTransform(R, T, s), iterations)
