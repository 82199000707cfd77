"""Float64 restatement of mesh_renderer.points.nearest_triangles / point_mesh_distance, written from the definition
("Point-cloud losses"): brute force over all N x T pairs on the float32 inputs promoted to float64,
and the seeded meshes and clouds the host and the GPU tests share.

  dist^2(p, (a, b, c)), e0 = b - a, e1 = c - a, d = p - a, det = |e0|^2 |e1|^2 - (e0.e1)^2: the least of
    - the plane projection a + v e0 + w e1 when det > 0 and v >= 0, w >= 0, v + w <= 1
    - the closest points of the segments ab, bc, ca (parameter clamped to [0, 1]; a zero-length segment: its end)
  each as |d - (beta e0 + gamma e1)|^2.  A triangle with an index outside [0, V) is never chosen; a padded query and
  a query without any distance below +inf give 0 / -1 / 0.

Forward tolerance.  The unit is 2^-24 * scale_i, scale_i = max_k |p_i - v_k|^2 over the corners of the face
concerned, in float64.  HOST_WORST_UNITS is the worst error of the package's float32 torch path on the CPU against
this restatement over every shape below, the translated case and the all-degenerate mesh: 1.74 units on the minima
(shape 2; 1e-9 on the distance to the named face, 1.74 on the distance at the barycentrics).  The host test holds
the torch path to 2 x that (3.48 units), the HIP kernels get 4 x that (6.96 units), because FMA contraction and the
reciprocal spelling reorder the rounding.

The distance at the returned barycentrics is checked in two float64 spellings.  |p - sum_k bary_k v_k|^2 multiplies
the float32 rounding of the barycentrics (their sum is 1 only within an ulp) by |v|, so it can hold to 2 atol only
where the mesh sits in the unit cube: there it is asserted.  Its difference form, |(p - v_0) - (bary_1 (v_1 - v_0) +
bary_2 (v_2 - v_0))|^2 -- the same number when the sum is exactly 1 -- is asserted everywhere, the translated case
included (measured there on the torch path: 11.6 units in the first spelling, 0.5 in the second).
"""
import numpy as np
import torch

# (B, N, V, T) of mesh k, seeded numpy.random.default_rng(300 + k).  0..5: the issue's list.  6..8: one query above
# queries_per_lane x workgroup size of nearest_triangle_plan (1 x 256, 2 x 256) and one triangle above its tile
# (128); 8 is the two-queries-a-lane kernel without a split.
SHAPES = [(1, 1, 3, 1), (1, 1, 40, 300), (2, 300, 3, 1), (3, 65, 30, 63), (2, 257, 200, 1031), (1, 40, 900, 5000),
          (1, 257, 50, 129), (2, 513, 60, 129), (1, 520, 40, 100)]
HOST_WORST_UNITS = 1.74                  # measured, see above
HOST_BOUND_UNITS = 2 * HOST_WORST_UNITS   # the float32 torch path
HIP_BOUND_UNITS = 4 * HOST_WORST_UNITS    # the HIP kernels
UNIT = 2.0 ** -24

_meshes = {}
_nearest = {}
INF = float("inf")


def _build(rng, B, N, V, T, offset=None):
    v = rng.uniform(-1, 1, (B, V, 3))
    p = rng.uniform(-1, 1, (B, N, 3))
    if offset is not None:
        v, p = v + np.asarray(offset), p + np.asarray(offset)
    tri = rng.integers(0, V, (T, 3))
    if T >= 8:   # degenerate triangles and an exact copy among the ordinary ones
        tri[2] = [tri[2][0], tri[2][0], tri[2][2]]
        tri[4] = [tri[4][1]] * 3
        tri[6] = tri[1]
    return (torch.from_numpy(p.astype(np.float32)), torch.from_numpy(v.astype(np.float32)),
            torch.from_numpy(tri.astype(np.int64)))


def mesh(k):
    """-> (points [B,N,3] f32, vertices [B,V,3] f32, triangles [T,3] i64) of shape k or "translated", built once."""
    if k not in _meshes:
        if k == "translated":   # where a distance from absolute coordinates loses its digits
            _meshes[k] = _build(np.random.default_rng(7), 1, 500, 120, 700, offset=(100.0, -50.0, 25.0))
        else:
            _meshes[k] = _build(np.random.default_rng(300 + k), *SHAPES[k])
    return _meshes[k]


def degenerate_mesh():
    """(2, 90, 12, 40): nothing but zero-area triangles -- two equal indices, three equal indices, three points on a
    line (b the midpoint of a and c, exact in float32)."""
    rng = np.random.default_rng(41)
    v = rng.integers(-8, 9, (2, 12, 3)).astype(np.float64) / 8.0
    v[:, 11] = (v[:, 9] + v[:, 10]) / 2.0
    tri = rng.integers(0, 9, (40, 3))
    tri[:, 1] = tri[:, 0]
    tri[::3, 2] = tri[::3, 0]
    tri[1] = [9, 11, 10]
    tri[7] = [10, 9, 11]
    p = rng.uniform(-1, 1, (2, 90, 3))
    return (torch.from_numpy(p.astype(np.float32)), torch.from_numpy(v.astype(np.float32)), torch.from_numpy(tri))


def sliver_mesh():
    """(2, 300, 180, 60): separate triangles that are thin but not degenerate -- c lies within 1e-7 .. 1e-2 of the line
    ab.  The projection's coordinates come from float32 dot products scaled by 1 / det, so on such a triangle they can
    be far from the true projection and still pass the inside test (check_sliver states what holds then)."""
    rng = np.random.default_rng(43)
    a, b = rng.uniform(-1, 1, (2, 60, 3)), rng.uniform(-1, 1, (2, 60, 3))
    along, across = rng.uniform(-0.5, 1.5, (2, 60, 1)), rng.normal(size=(2, 60, 3))
    c = a + along * (b - a) + 10.0 ** rng.uniform(-7, -2, (2, 60, 1)) * across
    v = np.stack([a, b, c], 2).reshape(2, 180, 3)
    p = rng.uniform(-1, 1, (2, 300, 3))
    return (torch.from_numpy(p.astype(np.float32)), torch.from_numpy(v.astype(np.float32)),
            torch.arange(180).reshape(60, 3))


def _sq(x):
    return (x * x).sum(-1)


def _segment(d, e):
    """Closest point of the segment from the origin to e, to d -> parameter in [0, 1] (0 for a zero-length one)."""
    ee = _sq(e)
    t = torch.where(ee > 0, (d * e).sum(-1) / torch.where(ee > 0, ee, torch.ones_like(ee)), torch.zeros_like(ee))
    return t.clamp(0, 1)


def closest(p, a, b, c, boundary_only=False):
    """float64 tensors that broadcast to [...,3] -> (dist^2 [...], barycentrics [...,3]) by the definition;
    boundary_only: of the three segments alone."""
    e0, e1, d = b - a, c - a, p - a
    d00, d01, d11 = _sq(e0), (e0 * e1).sum(-1), _sq(e1)
    det = d00 * d11 - d01 * d01
    p0, p1 = (d * e0).sum(-1), (d * e1).sum(-1)
    safe = torch.where(det > 0, det, torch.ones_like(det))
    v, w = (d11 * p0 - d01 * p1) / safe, (d00 * p1 - d01 * p0) / safe
    inside = (det > 0) & (v >= 0) & (w >= 0) & (v + w <= 1) & (not boundary_only)
    zero = torch.zeros_like(p0)
    tab, tca = _segment(d, e0), _segment(d, e1)
    tbc = _segment(d - e0, e1 - e0)
    beta = torch.stack([torch.where(inside, v, zero), tab, 1.0 - tbc, zero], -1)
    gamma = torch.stack([torch.where(inside, w, zero), zero, tbc, tca], -1)
    dist = _sq(d[..., None, :] - (beta[..., None] * e0[..., None, :] + gamma[..., None] * e1[..., None, :]))
    always = torch.ones_like(inside)
    dist = torch.where(torch.stack([inside, always, always, always], -1), dist, torch.full_like(dist, INF))
    best = dist.min(dim=-1)
    pick = best.indices[..., None]
    be, ga = torch.gather(beta, -1, pick)[..., 0], torch.gather(gamma, -1, pick)[..., 0]
    return best.values, torch.stack([1.0 - be - ga, be, ga], -1)


def _valid(lengths, B, n):
    if lengths is None:
        return torch.full((B,), n, dtype=torch.int64)
    return torch.as_tensor(lengths).long().cpu().clamp(0, n)


def all_distances(points, vertices, triangles, boundary_only=False):
    """[B,N,T] float64, +inf for a triangle with an index outside [0, V) (differentiable in float64 inputs);
    boundary_only: to the triangles' edges."""
    p, v, tri = points.double(), vertices.double(), triangles.long()
    V = v.shape[1]
    usable = ((tri >= 0) & (tri < V)).all(dim=1)
    a, b, c = (v[:, tri[:, k].clamp(0, V - 1)][:, None] for k in range(3))   # [B,1,T,3]
    dist, _ = closest(p[:, :, None, :], a, b, c, boundary_only)
    return torch.where(usable[None, None, :], dist, torch.full_like(dist, INF))


def nearest(points, vertices, triangles, lengths=None):
    """-> (min [B,N] f64, the first face attaining it [B,N] i64); 0 / -1 for rows without a result."""
    B, N = points.shape[:2]
    d = all_distances(points, vertices, triangles)
    d = torch.where(d == d, d, torch.full_like(d, INF))
    face = torch.from_numpy(np.argmin(d.numpy(), axis=2))   # numpy: the first of equal minima
    best = torch.gather(d, 2, face[..., None])[..., 0]
    valid = (torch.arange(N)[None, :] < _valid(lengths, B, N)[:, None]) & (best < INF)
    return torch.where(valid, best, torch.zeros_like(best)), torch.where(valid, face, torch.full_like(face, -1))


def cached_nearest(k):
    if k not in _nearest:
        _nearest[k] = nearest(*mesh(k))
    return _nearest[k]


def _corners(vertices, triangles, face):
    """[B,N,3(corner),3] float64 of the given faces (face -1 reads face 0)."""
    v, tri = vertices.double(), triangles.long()
    which = tri.clamp(0, v.shape[1] - 1)[face.long().clamp(min=0)]                       # [B,N,3]
    return torch.stack([torch.gather(v, 1, which[..., k, None].expand(-1, -1, 3)) for k in range(3)], 2)


def distance_to_face(points, vertices, triangles, face):
    """-> (dist^2 [B,N] f64 to the GIVEN face, its barycentrics [B,N,3]); 0 where face is -1."""
    c = _corners(vertices, triangles, face)
    dist, bary = closest(points.double(), c[:, :, 0], c[:, :, 1], c[:, :, 2])
    have = face.long() >= 0
    return torch.where(have, dist, torch.zeros_like(dist)), torch.where(have[..., None], bary, torch.zeros_like(bary))


def scale(points, vertices, triangles, face):
    """max_k |p_i - v_k|^2 over the corners of the given face, [B,N] f64."""
    c = _corners(vertices, triangles, face)
    return _sq(points.double()[:, :, None, :] - c).max(dim=2).values


def distance_at(points, vertices, triangles, face, bary):
    """|p_i - sum_k bary_ik v_k|^2 in float64 for the GIVEN face and barycentrics; 0 where face is -1
    (differentiable in float64 points / vertices)."""
    c = _corners(vertices, triangles, face)
    diff = points.double() - (bary.double()[..., None] * c).sum(2)
    return torch.where(face.long() >= 0, _sq(diff), torch.zeros(face.shape, dtype=torch.float64))


def distance_at_relative(points, vertices, triangles, face, bary):
    """distance_at in the difference form relative to the first corner: equal to it when the barycentrics add up to
    exactly 1."""
    c = _corners(vertices, triangles, face)
    w = bary.double()
    diff = (points.double() - c[:, :, 0]) - (w[..., 1:2] * (c[:, :, 1] - c[:, :, 0]) + w[..., 2:3] * (c[:, :, 2] - c[:, :, 0]))
    return torch.where(face.long() >= 0, _sq(diff), torch.zeros(face.shape, dtype=torch.float64))


def gradients(points, vertices, triangles, face, bary, upstream):
    """The float64 gradients of sum_i upstream_i |p_i - c_i|^2 for the GIVEN (face, bary) held constant ->
    (dpoints, dvertices)."""
    p, v = points.double().clone().requires_grad_(True), vertices.double().clone().requires_grad_(True)
    (distance_at(p, v, triangles, face, bary) * upstream.double()).sum().backward()
    return p.grad, v.grad


def mean_of(sqdist, lengths=None):
    B, N = sqdist.shape
    nv = _valid(lengths, B, N)
    return sqdist.double().sum(1) / nv.clamp(min=1).double()


def mean_atol(points, vertices, triangles, face, bound_units, lengths=None):
    """The mean over each image's valid rows of atol_i = bound x 2^-24 x scale_i for the given faces, [B] f64."""
    atol = bound_units * UNIT * scale(points, vertices, triangles, face)
    return mean_of(torch.where(face.long() >= 0, atol, torch.zeros_like(atol)), lengths)


def mean_gradients(points, vertices, triangles, face, bary, upstream, lengths=None):
    """The float64 gradients of sum_b upstream_b mean_b for the GIVEN (face, bary)."""
    p, v = points.double().clone().requires_grad_(True), vertices.double().clone().requires_grad_(True)
    (mean_of(distance_at(p, v, triangles, face, bary), lengths) * upstream.double()).sum().backward()
    return p.grad, v.grad


def gradients_through_the_min(points, vertices, triangles, upstream):
    """float64 autograd through the brute-force minimum itself (no envelope theorem) -> (dpoints, dvertices)."""
    p, v = points.double().clone().requires_grad_(True), vertices.double().clone().requires_grad_(True)
    (all_distances(p, v, triangles).min(dim=2).values * upstream.double()).sum().backward()
    return p.grad, v.grad


def check_forward(errors, bound_units, what, in_unit_cube=True):
    """The forward assertions on forward_errors()' figures, printed first."""
    print("%s: %s (bound %.2f units)" % (what, {k: float("%.3g" % v) for k, v in errors.items()}, bound_units))
    assert errors["min"] <= bound_units, "%s: sqdist is %.3g units from the minimum" % (what, errors["min"])
    assert errors["face"] <= bound_units, "%s: the named face is %.3g units from nearest" % (what, errors["face"])
    assert errors["bary_relative"] <= 2 * bound_units, what
    if in_unit_cube:
        assert errors["bary"] <= 2 * bound_units, what
    assert errors["low"] >= 0.0 and errors["sum"] <= 4 * 2.0 ** -23, "%s: barycentrics" % what


def check_sliver(points, vertices, triangles, sqdist, face, bary, bound_units, what):
    """What holds on thin triangles whatever the projection's coordinates lost: the result is the distance to a
    point of the named triangle (the float64 distance at the returned barycentrics is sqdist within 2 atol, the
    barycentrics are >= 0 and add up to 1), so it is never below the true minimum by more than atol, and the
    segment candidates keep it from exceeding the nearest EDGE's distance by more than atol.  The excess over the
    true minimum is printed, not asserted: the torch path reaches 19.6 units on this mesh, the kernels 8.7."""
    errors = forward_errors(points, vertices, triangles, sqdist, face, bary)
    print("%s: %s (bound %.2f units)" % (what, {k: float("%.3g" % v) for k, v in errors.items()}, bound_units))
    got, named = sqdist.detach().double().cpu(), face.cpu().long()
    atol = bound_units * UNIT * scale(points, vertices, triangles, named)
    want, _ = nearest(points, vertices, triangles)
    edges = all_distances(points, vertices, triangles, boundary_only=True).min(dim=2).values
    assert bool((got >= want - atol).all()), "%s: below the true minimum" % what
    assert bool((got <= edges + atol).all()), "%s: above the nearest edge" % what
    assert errors["bary_relative"] <= 2 * bound_units and errors["bary"] <= 2 * bound_units, what
    assert errors["low"] >= 0.0 and errors["sum"] <= 4 * 2.0 ** -23, "%s: barycentrics" % what


def forward_errors(points, vertices, triangles, sqdist, face, bary, lengths=None):
    """Every forward check of one result against the restatement, in units of 2^-24 * scale_i ->
    {"min": worst |sqdist - ref_min|, "face": worst excess of ref_dist(p, face) over ref_min, "bary": worst
    | |p - sum bary v|^2 - sqdist | (its bound is twice the others'), "bary_relative": the same in the difference
    form, "sum": worst |sum bary - 1|, "low": least bary}
    over the rows with a face; asserts that exactly the reference's rows have one."""
    want, want_face = nearest(points, vertices, triangles, lengths)
    sqdist, face, bary = sqdist.detach().double().cpu(), face.cpu().long(), bary.detach().double().cpu()
    have = want_face >= 0
    assert torch.equal(face >= 0, have), "rows with a result differ from the restatement's"
    assert bool((face[~have] == -1).all()) and bool((sqdist[~have] == 0).all()) and bool((bary[~have] == 0).all())
    assert bool((face < triangles.shape[0]).all())
    if not bool(have.any()):
        return {"min": 0.0, "face": 0.0, "bary": 0.0, "bary_relative": 0.0, "sum": 0.0, "low": 0.0}
    to_named, _ = distance_to_face(points, vertices, triangles, face)
    unit = UNIT * scale(points, vertices, triangles, face)
    at = distance_at(points, vertices, triangles, face, bary)
    relative = distance_at_relative(points, vertices, triangles, face, bary)
    pick = lambda t: float(t[have].max())
    return {"min": pick((sqdist - want).abs() / unit), "face": pick((to_named - want) / unit),
            "bary": pick((at - sqdist).abs() / unit), "bary_relative": pick((relative - sqdist).abs() / unit), "sum": pick((bary.sum(-1) - 1).abs()),
            "low": float(bary[have].min())}
