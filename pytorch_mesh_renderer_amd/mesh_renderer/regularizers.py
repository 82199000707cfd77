"""Mesh regularisers: uniform Laplacian smoothing, edge length and normal consistency.

What keeps a deforming mesh usable while a silhouette or image loss pulls on its vertices ("Mesh
regularisers").  The first two are the terms of the reference's mesh-fitting example (src/examples/example7b.py:
17-129, a sparse matrix product and fancy-indexed gathers in eager torch); the third is the term mesh fitting
commonly adds.  On a HIP device the three share one topology (mesh_topology(), cached on the triangle tensor), one
forward launch, a small fixed-order sum and one backward launch (csrc/mesh_reg.hip: gathers, no atomics, bitwise
reproducible).  Host tensors and tensors that are not float32 -- mesh preparation, the CPU test-suite -- take the
equivalent batched torch expression over the same topology.
"""
import torch

from .. import _native
from .._native import MESH_EDGE, MESH_LAPLACIAN, MESH_NORMAL

NORMAL_FLOOR = 1e-8   # a flap with |n0| or |n1| at or below this has value 0 and gradient 0


def mesh_topology(triangles, vertex_count):
    """The topology the regularisers run on, of triangles [T,3] (any integer dtype) for `vertex_count` vertices: an
    object with edges [E,2], nbr_offsets [V+1], nbr [2E], flaps [F,4], role_offsets [V+1], roles [4F] (int32, on the
    triangles' device) and vertex_count, edge_count, flap_count.  Computed once per triangle tensor (cached on the
    tensor object, keyed by its version counter)."""
    _integer_triangles(triangles)
    return _native.mesh_topology(triangles, int(vertex_count))


def _integer_triangles(triangles):
    if not torch.is_tensor(triangles):
        raise TypeError("triangles must be a tensor")
    if triangles.dtype in (torch.float16, torch.float32, torch.float64, torch.bfloat16, torch.bool):
        raise RuntimeError("triangles must hold integer vertex indices")
    if triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [*, 3], got %s" % list(triangles.shape))


class _MeshTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, topology, terms, target_length):
        v = vertices.detach().contiguous()
        out, unit_dirs = _native.mesh_regularizer_forward(v, topology, terms, target_length)
        # the topology travels with the node: the backward does not rebuild it when the cache on the caller's
        # tensor object is gone
        ctx.topology, ctx.terms, ctx.target_length = topology, terms, target_length
        ctx.save_for_backward(v, unit_dirs)
        return out

    @staticmethod
    def backward(ctx, dterms):
        v, unit_dirs = ctx.saved_tensors
        dvertices = _native.mesh_regularizer_backward(dterms.contiguous(), v, unit_dirs, ctx.topology, ctx.terms,
                                                      ctx.target_length)
        return dvertices, None, None, None


def _safe_norm(x):
    """|x| over the last axis with gradient 0 where x = 0."""
    sq = (x * x).sum(-1)
    nonzero = sq > 0
    return torch.where(nonzero, torch.sqrt(torch.where(nonzero, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def _terms_torch(vertices, topology, terms, target_length):
    """The three terms as a batched torch expression on the device and in the dtype of `vertices` [B,V,3]."""
    B, V, _ = vertices.shape
    zero = vertices.new_zeros(B)
    lap, edge, nc = zero, zero, zero
    edges = topology.edges.to(vertices.device).long()
    flaps = topology.flaps.to(vertices.device).long()
    lo, hi = edges[:, 0], edges[:, 1]
    if terms & MESH_LAPLACIAN:
        src, dst = torch.cat([lo, hi]), torch.cat([hi, lo])
        # the sum of v_j - v_i, as the kernel forms it: nothing cancels against |v| far from the origin
        sums = torch.zeros_like(vertices).index_add(
            1, src, vertices.index_select(1, dst) - vertices.index_select(1, src))
        degree = torch.zeros(V, dtype=vertices.dtype, device=vertices.device).index_add_(
            0, src, torch.ones(src.shape[0], dtype=vertices.dtype, device=vertices.device))
        delta = sums / degree.clamp(min=1)[None, :, None]
        lap = _safe_norm(delta).sum(1) / V
    if terms & MESH_EDGE and edges.shape[0] > 0:
        length = _safe_norm(vertices.index_select(1, lo) - vertices.index_select(1, hi))
        edge = (length if target_length is None else (length - float(target_length)) ** 2).mean(1)
    if terms & MESH_NORMAL and flaps.shape[0] > 0:
        a, b, c, d = [vertices.index_select(1, flaps[:, k]) for k in range(4)]
        n0 = torch.cross(b - a, c - a, dim=-1)
        n1 = torch.cross(d - a, b - a, dim=-1)
        l0, l1 = _safe_norm(n0), _safe_norm(n1)
        ok = (l0 > NORMAL_FLOOR) & (l1 > NORMAL_FLOOR)
        # 1 - cos as |h0 - h1|^2 / 2 on the unit normals: no cancellation against 1 on a nearly flat flap
        one = torch.ones_like(l0)
        h = n0 / torch.where(ok, l0, one)[..., None] - n1 / torch.where(ok, l1, one)[..., None]
        nc = torch.where(ok, 0.5 * (h * h).sum(-1), torch.zeros_like(l0)).mean(1)
    return torch.stack([lap, edge, nc], dim=1)


def _terms(vertices, triangles, terms, target_length):
    """-> ([B,3], whether `vertices` came without the batch axis)."""
    if not torch.is_tensor(vertices) or not vertices.is_floating_point():
        raise TypeError("vertices must be a floating-point tensor")
    single = vertices.dim() == 2
    v = vertices.unsqueeze(0) if single else vertices
    if v.dim() != 3 or v.shape[2] != 3 or v.shape[1] < 1:
        raise ValueError("vertices must have shape [B, V, 3] or [V, 3] with V >= 1, got %s" % list(vertices.shape))
    _integer_triangles(triangles)
    if target_length is not None:
        target_length = float(target_length)
    if triangles.device != v.device:
        triangles = triangles.to(v.device)
    topology = _native.mesh_topology(triangles, v.shape[1])
    if v.is_cuda and v.dtype == torch.float32:
        return _MeshTerms.apply(v, topology, int(terms), target_length), single
    return _terms_torch(v, topology, int(terms), target_length), single


def mesh_terms(vertices, triangles, laplacian=True, edge=True, normal=True, target_length=None):
    """vertices [B,V,3] (or [V,3]: one image), triangles [T,3] of any integer dtype, one topology for the batch
    -> [B,3]: (Laplacian, edge length, normal consistency) per image.  A term switched off is not computed and
    reads 0.  target_length None: the mean edge length; a float: the mean of (length - target_length)^2.
    Differentiable to the vertices."""
    mask = (MESH_LAPLACIAN if laplacian else 0) | (MESH_EDGE if edge else 0) | (MESH_NORMAL if normal else 0)
    return _terms(vertices, triangles, mask, target_length)[0]


def _one_term(vertices, triangles, mask, column, target_length=None):
    terms, single = _terms(vertices, triangles, mask, target_length)
    return terms[0, column] if single else terms[:, column]


def laplacian_smoothing(vertices, triangles):
    """Uniform Laplacian: the mean over ALL vertices of |mean of the neighbours - the vertex| (a vertex without
    neighbours contributes 0) -> [B], or a 0-dim tensor for [V,3] vertices."""
    return _one_term(vertices, triangles, MESH_LAPLACIAN, 0)


def edge_length(vertices, triangles, target_length=None):
    """The mean length of the unique edges, or with a float target_length the mean of (length - target_length)^2
    -> [B], or a 0-dim tensor for [V,3] vertices."""
    return _one_term(vertices, triangles, MESH_EDGE, 1, target_length)


def normal_consistency(vertices, triangles):
    """The mean of 1 - cos(angle between the two face normals) over the edges that exactly two triangles share: 0
    where the surface is flat, 2 at a fold-back, whatever the triangles' winding -> [B], or a 0-dim tensor for
    [V,3] vertices."""
    return _one_term(vertices, triangles, MESH_NORMAL, 2)


def mesh_regularizer(vertices, triangles, laplacian=0.0, edge=0.0, normal=0.0, target_length=None):
    """laplacian * lap + edge * edge_length + normal * nc per image -> [B] (a 0-dim tensor for [V,3] vertices).
    The weights are Python numbers; a term whose weight is 0 is not computed."""
    weights = [float(laplacian), float(edge), float(normal)]
    mask = sum(bit for bit, w in zip((MESH_LAPLACIAN, MESH_EDGE, MESH_NORMAL), weights) if w != 0.0)
    terms, single = _terms(vertices, triangles, mask, target_length)
    total = (terms * _weight_row(weights, terms)).sum(1)
    return total[0] if single else total


_weight_rows = {}


def _weight_row(weights, like):
    """[3] weights on the device and in the dtype of `like`, uploaded once per value: a step that is captured into a
    HIP graph (capture_step) must not upload anything, and its warm-up steps fill this cache."""
    key = (tuple(weights), like.device, like.dtype)
    row = _weight_rows.get(key)
    if row is None:
        if len(_weight_rows) >= 64:
            _weight_rows.clear()
        row = _weight_rows[key] = torch.tensor(weights, dtype=like.dtype, device=like.device)
    return row
