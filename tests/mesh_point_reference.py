"""Float64 restatement of mesh_renderer.points.triangle_nearest_points / mesh_point_distance, the other direction of
tests/point_mesh_reference.py (imported, not changed): the same brute force over all N x T pairs by the definition at
the top of that module, reduced over the POINT axis, and the seeded shapes the host and the GPU tests share.

  sqdist_t = min over the valid points j of dist^2(p_j, triangle t),  index_t = the first j that attains it;
  a triangle with an index outside [0, V) and a triangle without any distance below +inf give 0 / -1 / 0.

A result row is a triangle; its pair is (point index_t, triangle t).  point_mesh_reference's per-row functions take
a point and a face per row, so they serve here with the chosen points gathered and face = t (pair_rows()).

Forward tolerance.  The unit is the existing one, 2^-24 * scale, scale = max_k |p_j - v_k|^2 over the corners of the
pair concerned, in float64.  HOST_WORST_UNITS is the worst error of the package's float32 torch path on the CPU
against this restatement over CASES (point_mesh_reference's shapes, the translated case, the all-degenerate mesh,
the shapes below; the sliver mesh is held to check_sliver's weaker statement instead, as there): 2.25 units on the
minima, on the all-degenerate mesh (1.92 on point_mesh_reference's shape 1, below 1.4 elsewhere; 0 on the distance
to the named pair; 2.25 on the distance at the barycentrics, whose bound is twice the others').
The host test holds the torch path to 2 x that, the HIP kernels get 4 x that, by point_mesh_reference's reasoning:
FMA contraction and the reciprocal spelling reorder the rounding.
"""
import numpy as np
import torch

import point_mesh_reference as ref

# (B, N, V, T), seeded numpy.random.default_rng(500 + k) -- chosen from mr_nearest_point_of_triangle_plan: a point
# tile of 256, 256 triangles a workgroup, packed pairs from 256 points, 1024 workgroups wanted.
#   0: one point above the tile, an odd count: two splits, the second one lone point
#   1: several tiles inside ONE split (256 images x 1 workgroup want 4 splits of the 6 tiles: 3 of 2 tiles), the last
#      tile one lone point
#   2: one triangle above a workgroup of triangles
#   3: a small mesh against a large cloud: 9 splits          4: the same mesh, 256 points: packed, no split
#   5: the same mesh, 200 points: one point a step, no split  6: per-image lengths (LENGTHS), one 0 and one odd
SHAPES = [(1, 257, 40, 50), (256, 1281, 8, 3), (1, 300, 60, 257), (1, 2049, 30, 7), (1, 256, 30, 7), (1, 200, 30, 7),
          (3, 700, 40, 90)]
LENGTHS = {6: [700, 0, 333]}
# every case that is held to the bound: ("ref", k) is point_mesh_reference.mesh(k), ("own", k) is SHAPES[k]
CASES = ([("ref", k) for k in range(len(ref.SHAPES))] + [("ref", "translated"), ("ref", "degenerate")]
         + [("own", k) for k in range(len(SHAPES))])
HOST_WORST_UNITS = 2.25                  # measured, see above
HOST_WORST_CASE = ("ref", "degenerate")
HOST_BOUND_UNITS = 2 * HOST_WORST_UNITS   # the float32 torch path
HIP_BOUND_UNITS = 4 * HOST_WORST_UNITS    # the HIP kernels
UNIT = ref.UNIT
INF = float("inf")

_meshes = {}
_nearest = {}


def case(c):
    """-> (points, vertices, triangles, lengths or None) of a case, built once."""
    if c not in _meshes:
        kind, k = c
        if kind == "own":
            _meshes[c] = ref._build(np.random.default_rng(500 + k), *SHAPES[k]) + (
                torch.tensor(LENGTHS[k]) if k in LENGTHS else None,)
        elif k == "degenerate":
            _meshes[c] = ref.degenerate_mesh() + (None,)
        else:
            _meshes[c] = ref.mesh(k) + (None,)
    return _meshes[c]


def name(c):
    return "%s-%s" % c


def masked_distances(points, vertices, triangles, lengths=None, boundary_only=False):
    """ref.all_distances [B,N,T] with the rows beyond lengths and every NaN at +inf."""
    B, N = points.shape[:2]
    d = ref.all_distances(points, vertices, triangles, boundary_only)
    d = torch.where(d == d, d, torch.full_like(d, INF))
    padded = torch.arange(N)[None, :] >= ref._valid(lengths, B, N)[:, None]
    return d.masked_fill(padded[:, :, None], INF)


def nearest(points, vertices, triangles, lengths=None):
    """-> (min [B,T] f64, the first point attaining it [B,T] i64, the runner-up's excess over it [B,T], +inf with
    fewer than two distances below +inf); 0 / -1 for rows without a result."""
    d = masked_distances(points, vertices, triangles, lengths)
    index = torch.from_numpy(np.argmin(d.numpy(), axis=1))   # numpy: the first of equal minima
    best = torch.gather(d, 1, index[:, None, :])[:, 0]
    if d.shape[1] > 1:
        second = d.topk(2, dim=1, largest=False).values[:, 1]
        gap = torch.where(second < INF, second - best, torch.full_like(best, INF))
    else:
        gap = torch.full_like(best, INF)
    valid = best < INF
    return (torch.where(valid, best, torch.zeros_like(best)), torch.where(valid, index, torch.full_like(index, -1)),
            gap)


def cached_nearest(c):
    if c not in _nearest:
        _nearest[c] = nearest(*case(c))
    return _nearest[c]


def pair_rows(points, triangles, index):
    """The pairs (point index_t, triangle t) as rows for point_mesh_reference: (the chosen points [B,T,3], face
    [B,T] = t, -1 where index is)."""
    index = index.long()
    chosen = torch.gather(points, 1, index.clamp(min=0)[..., None].expand(-1, -1, 3))
    face = torch.arange(triangles.shape[0])[None, :].expand_as(index)
    return chosen, torch.where(index >= 0, face, torch.full_like(face, -1))


def scale(points, vertices, triangles, index):
    chosen, face = pair_rows(points, triangles, index)
    return ref.scale(chosen, vertices, triangles, face)


def usable_count(vertices, triangles):
    tri = triangles.long()
    return int(((tri >= 0) & (tri < vertices.shape[1])).all(dim=1).sum())


def mean_of(sqdist, vertices, triangles):
    """The sum over the triangles / U, [B] f64; 0 where U = 0 (rows without a result are 0 already)."""
    return sqdist.double().sum(1) / max(usable_count(vertices, triangles), 1)


def mean_atol(points, vertices, triangles, index, bound_units):
    atol = bound_units * UNIT * scale(points, vertices, triangles, index)
    return mean_of(torch.where(index.long() >= 0, atol, torch.zeros_like(atol)), vertices, triangles)


def gradients(points, vertices, triangles, index, bary, upstream):
    """The float64 gradients of sum_t upstream_t |p_index_t - c_t|^2 for the GIVEN (index, bary) held constant ->
    (dpoints, summed per point, dvertices).  The distance is taken in the difference form relative to the first
    corner (point_mesh_reference.distance_at_relative): |p - sum_k bary_k v_k|^2 multiplies the float32 rounding of
    the barycentrics' sum by |v|, which on the translated case is 1e-4 of these gradients by itself."""
    p, v = points.double().clone().requires_grad_(True), vertices.double().clone().requires_grad_(True)
    chosen, face = pair_rows(p, triangles, index)
    (ref.distance_at_relative(chosen, v, triangles, face, bary) * upstream.double()).sum().backward()
    return p.grad, v.grad


def mean_gradients(points, vertices, triangles, index, bary, upstream):
    """The float64 gradients of sum_b upstream_b mean_b for the GIVEN (index, bary)."""
    p, v = points.double().clone().requires_grad_(True), vertices.double().clone().requires_grad_(True)
    chosen, face = pair_rows(p, triangles, index)
    (mean_of(ref.distance_at_relative(chosen, v, triangles, face, bary), vertices, triangles) * upstream.double()).sum().backward()
    return p.grad, v.grad


def forward_errors(points, vertices, triangles, sqdist, index, bary, lengths=None, bound_units=None):
    """Every forward check of one result against the restatement, in units of 2^-24 * scale of the named pair ->
    {"min": worst |sqdist - ref_min|, "pair": worst excess of ref_dist(p_index, triangle) over ref_min, "bary": worst
    | |p - sum bary v|^2 - sqdist | (its bound is twice the others'), "bary_relative": the same in the difference
    form, "sum": worst |sum bary - 1|, "low": least bary, "index": with bound_units, the rows whose index differs from
    the restatement's although its minimum is separated from the runner-up by more than the bound}
    over the rows with a result; asserts that exactly the reference's rows have one and that every index is a valid
    point's."""
    B, N = points.shape[:2]
    want, want_index, gap = nearest(points, vertices, triangles, lengths)
    sqdist, index, bary = sqdist.detach().double().cpu(), index.cpu().long(), bary.detach().double().cpu()
    have = want_index >= 0
    assert torch.equal(index >= 0, have), "rows with a result differ from the restatement's"
    assert bool((index[~have] == -1).all()) and bool((sqdist[~have] == 0).all()) and bool((bary[~have] == 0).all())
    assert bool((index < ref._valid(lengths, B, N)[:, None]).all())
    zero = {"min": 0.0, "pair": 0.0, "bary": 0.0, "bary_relative": 0.0, "sum": 0.0, "low": 0.0, "index": 0}
    if not bool(have.any()):
        return zero
    chosen, face = pair_rows(points, triangles, index)
    to_named, _ = ref.distance_to_face(chosen, vertices, triangles, face)
    unit = UNIT * ref.scale(chosen, vertices, triangles, face)
    at = ref.distance_at(chosen, vertices, triangles, face, bary)
    relative = ref.distance_at_relative(chosen, vertices, triangles, face, bary)
    pick = lambda t: float(t[have].max())
    wrong = 0
    if bound_units is not None:
        want_unit = UNIT * scale(points, vertices, triangles, want_index)
        wrong = int((have & (gap > bound_units * want_unit) & (index != want_index)).sum())
    return {"min": pick((sqdist - want).abs() / unit), "pair": pick((to_named - want) / unit),
            "bary": pick((at - sqdist).abs() / unit), "bary_relative": pick((relative - sqdist).abs() / unit),
            "sum": pick((bary.sum(-1) - 1).abs()), "low": float(bary[have].min()), "index": wrong}


def check_forward(errors, bound_units, what, in_unit_cube=True):
    """The forward assertions on forward_errors()' figures, printed first."""
    print("%s: %s (bound %.2f units)" % (what, {k: float("%.3g" % v) for k, v in errors.items()}, bound_units))
    assert errors["min"] <= bound_units, "%s: sqdist is %.3g units from the minimum" % (what, errors["min"])
    assert errors["pair"] <= bound_units, "%s: the named point is %.3g units from nearest" % (what, errors["pair"])
    assert errors["index"] == 0, "%s: %d separated minima went to another point" % (what, errors["index"])
    assert errors["bary_relative"] <= 2 * bound_units, what
    if in_unit_cube:
        assert errors["bary"] <= 2 * bound_units, what
    assert errors["low"] >= 0.0 and errors["sum"] <= 4 * 2.0 ** -23, "%s: barycentrics" % what


def check_sliver(points, vertices, triangles, sqdist, index, bary, bound_units, what):
    """point_mesh_reference.check_sliver's statement for triangle rows, and no more: the result is the distance to a
    point of the triangle (the float64 distance at the returned barycentrics is sqdist within 2 atol, barycentrics
    >= 0 adding up to 1), never below the true minimum by more than atol, never above the distance from the
    triangle's nearest EDGE to its nearest point by more than atol.  The excess over the true minimum is printed."""
    errors = forward_errors(points, vertices, triangles, sqdist, index, bary)
    print("%s: %s (bound %.2f units)" % (what, {k: float("%.3g" % v) for k, v in errors.items()}, bound_units))
    got = sqdist.detach().double().cpu()
    atol = bound_units * UNIT * scale(points, vertices, triangles, index.cpu())
    want, _, _ = nearest(points, vertices, triangles)
    edges = masked_distances(points, vertices, triangles, boundary_only=True).min(dim=1).values
    assert bool((got >= want - atol).all()), "%s: below the true minimum" % what
    assert bool((got <= edges + atol).all()), "%s: above the nearest edge" % what
    assert errors["bary_relative"] <= 2 * bound_units and errors["bary"] <= 2 * bound_units, what
    assert errors["low"] >= 0.0 and errors["sum"] <= 4 * 2.0 ** -23, "%s: barycentrics" % what
