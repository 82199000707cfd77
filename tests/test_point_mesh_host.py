"""mesh_renderer.points.nearest_triangles / point_mesh_distance on the host: the chunked torch path against the
float64 restatement (tests/point_mesh_reference.py), the launch plan's invariants, the argument checks and the
envelope-theorem gradient against float64 autograd through the minimum.

Forward bound: ref.HOST_BOUND_UNITS (twice the torch path's own measured worst, 1.74) in units of 2^-24 * scale_i,
scale_i = max_k |p_i - v_k|^2 over the corners of the named face; gradients within 1e-4 of the largest magnitude of
the expected gradient tensor, the restatement being evaluated with the returned (face, bary)."""
import pytest
import torch

import point_mesh_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer

points = mesh_renderer.points
CASES = list(range(len(ref.SHAPES))) + ["translated"]


def _grad_close(got, want, what):
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    print("%s: gradient max err %.3g of scale %.3g" % (what, err, scale))
    assert err <= 1e-4 * scale, "%s: gradient error %.3g > 1e-4 * %.3g" % (what, err, scale)


def test_the_functions_are_exported():
    for name in ("nearest_triangles", "point_mesh_distance"):
        assert callable(getattr(mesh_renderer.points, name))


def test_the_shapes_cover_every_launch_path():
    plans = {shape: _native.nearest_triangle_plan(shape[0], shape[1], shape[3]) for shape in ref.SHAPES}
    assert plans[(1, 40, 900, 5000)]["splits"] > 1
    for lanes in (1, 2):   # both query widths, each with and without a split
        assert any(p["queries_per_lane"] == lanes and p["splits"] == 1 for p in plans.values())
        assert any(p["queries_per_lane"] == lanes and p["splits"] > 1 for p in plans.values())
    for p in plans.values():
        assert p["triangle_tile"] == 128 and p["workgroup_size"] == 256
    one, wide = plans[(1, 257, 50, 129)], plans[(2, 513, 60, 129)]
    assert one["queries_per_lane"] * one["workgroup_size"] + 1 == 257 and one["triangle_tile"] + 1 == 129
    assert wide["queries_per_lane"] * wide["workgroup_size"] + 1 == 513 and wide["triangle_tile"] + 1 == 129
    assert _native.nearest_triangle_plan(1, 512, 100)["queries_per_lane"] == 2
    assert _native.nearest_triangle_plan(1, 511, 100)["queries_per_lane"] == 1


def test_the_plan_has_no_empty_split_and_refuses_sizes_outside_the_limits():
    for B in (1, 2, 7, 32, 5000):
        for N in (1, 255, 256, 257, 511, 512, 513, 20000):
            for T in (1, 127, 128, 129, 1000, 5000, 49928):
                p = _native.nearest_triangle_plan(B, N, T)
                tile = p["triangle_tile"]
                tiles = -(-T // tile)
                chunk_tiles = -(-tiles // p["splits"])
                assert 1 <= p["splits"] <= tiles
                assert (p["splits"] - 1) * chunk_tiles < tiles       # the last split still has a tile
                assert p["queries_per_lane"] == (2 if N >= 512 else 1)
    for bad in ((0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, 1, 0), (1, (1 << 28) + 1, 1), (1, 1, (1 << 28) + 1),
                (65535, 1 << 21, 1), (-1, 5, 5)):
        with pytest.raises(ValueError):
            _native.nearest_triangle_plan(*bad)
    assert _native.nearest_triangle_plan(1, 1 << 28, 1 << 28)["splits"] >= 1


@pytest.mark.parametrize("k", CASES)
def test_torch_path_matches_the_restatement(k):
    p, v, tri = ref.mesh(k)
    pl, vl = p.clone().requires_grad_(True), v.clone().requires_grad_(True)
    sqdist, face, bary = points.nearest_triangles(pl, vl, tri)
    assert sqdist.shape == face.shape == p.shape[:2] and bary.shape == p.shape
    assert sqdist.dtype == bary.dtype == torch.float32 and face.dtype == torch.int32
    assert sqdist.grad_fn is not None and not face.requires_grad and not bary.requires_grad
    errors = ref.forward_errors(p, v, tri, sqdist, face, bary)
    ref.check_forward(errors, ref.HOST_BOUND_UNITS, "torch path %s" % (k,), in_unit_cube=k != "translated")
    g = torch.Generator().manual_seed(3)
    upstream = torch.randn(sqdist.shape, generator=g)
    sqdist.backward(upstream)
    wdp, wdv = ref.gradients(p, v, tri, face, bary, upstream)
    _grad_close(pl.grad, wdp, "%s dpoints" % (k,))
    _grad_close(vl.grad, wdv, "%s dvertices" % (k,))
    # the mean
    pl, vl = p.clone().requires_grad_(True), v.clone().requires_grad_(True)
    mean = points.point_mesh_distance(pl, vl, tri)
    assert mean.shape == (p.shape[0],) and mean.dtype == torch.float32
    want, want_face = ref.nearest(p, v, tri) if k == "translated" else ref.cached_nearest(k)
    want_mean = ref.mean_of(want)
    atol = ref.mean_atol(p, v, tri, want_face, ref.HOST_BOUND_UNITS)
    assert bool(((mean.detach().double() - want_mean).abs() <= 1e-5 * want_mean + atol).all())
    weights = torch.randn(p.shape[0], generator=g)
    mean.backward(weights)
    wdp, wdv = ref.mean_gradients(p, v, tri, face, bary, weights)
    _grad_close(pl.grad, wdp, "%s mean dpoints" % (k,))
    _grad_close(vl.grad, wdv, "%s mean dvertices" % (k,))


def test_the_envelope_gradient_is_the_gradient_through_the_minimum():
    """A case with clear margins: four separate triangles around the corners of a tetrahedron, so that a query whose
    closest point lies on an edge or a corner has no second face at the same distance; float64 on both sides."""
    g = torch.Generator().manual_seed(12)
    centres = 1.2 * torch.tensor([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]],
                                 dtype=torch.float64)
    v = (centres[:, None, :] + 0.6 * torch.randn(4, 3, 3, generator=g, dtype=torch.float64)).reshape(1, 12, 3)
    tri = torch.arange(12).reshape(4, 3)
    p = (torch.rand(1, 400, 3, generator=g, dtype=torch.float64) * 4 - 2)
    d = ref.all_distances(p, v, tri)
    runner_up = d.topk(2, dim=2, largest=False).values
    clear = (runner_up[..., 1] - runner_up[..., 0]) > 1e-3
    p = p[clear][None]
    assert p.shape[1] > 300
    pl, vl = p.clone().requires_grad_(True), v.clone().requires_grad_(True)
    sqdist, face, bary = points.nearest_triangles(pl, vl, tri)
    assert sqdist.dtype == torch.float64
    # interior, edge and corner rows are all present
    zeros = (bary == 0).sum(-1)
    assert bool((zeros == 0).any()) and bool((zeros == 1).any()) and bool((zeros == 2).any())
    upstream = torch.randn(sqdist.shape, generator=g, dtype=torch.float64)
    sqdist.backward(upstream)
    wdp, wdv = ref.gradients_through_the_min(p, v, tri, upstream)
    assert float((pl.grad - wdp).abs().max()) <= 1e-10 * float(wdp.abs().max())
    assert float((vl.grad - wdv).abs().max()) <= 1e-10 * float(wdv.abs().max())


def test_degenerate_triangles_alone():
    p, v, tri = ref.degenerate_mesh()
    pl, vl = p.clone().requires_grad_(True), v.clone().requires_grad_(True)
    sqdist, face, bary = points.nearest_triangles(pl, vl, tri)
    assert bool(torch.isfinite(sqdist).all()) and bool((face >= 0).all())
    ref.check_forward(ref.forward_errors(p, v, tri, sqdist, face, bary), ref.HOST_BOUND_UNITS, "degenerate mesh")
    sqdist.sum().backward()
    assert bool(torch.isfinite(pl.grad).all()) and bool(torch.isfinite(vl.grad).all())


def test_thin_triangles_stay_between_the_minimum_and_the_nearest_edge():
    p, v, tri = ref.sliver_mesh()
    sqdist, face, bary = points.nearest_triangles(p, v, tri)
    ref.check_sliver(p, v, tri, sqdist, face, bary, ref.HOST_BOUND_UNITS, "torch path, thin triangles")


def test_exact_ties_go_to_the_lowest_face():
    p, v, tri = ref.mesh(3)
    base = points.nearest_triangles(p, v, tri)
    again = points.nearest_triangles(p, v, torch.cat([tri, tri, tri]))
    for a, b in zip(base, again):
        assert torch.equal(a, b)


def test_lengths_unusable_triangles_and_non_finite_coordinates():
    p, v, tri = ref.mesh(4)
    B, N, V, T = ref.SHAPES[4]
    lengths = torch.tensor([100, 0])
    poisoned = p.clone()
    poisoned[0, 100:] = float("nan")
    poisoned[1] = float("nan")
    runs = []
    for cloud in (p, poisoned):
        pl, vl = cloud.clone().requires_grad_(True), v.clone().requires_grad_(True)
        out = points.nearest_triangles(pl, vl, tri, lengths)
        mean = points.point_mesh_distance(pl, vl, tri, lengths)
        (out[0].sum() + mean.sum()).backward()
        runs.append(tuple(t.detach() for t in out) + (mean.detach(), pl.grad, vl.grad))
    for a, b in zip(*runs):                    # the padding influences nothing, bit for bit
        assert torch.equal(a, b)
    sqdist, face, bary, mean, dp, dv = runs[0]
    ref.check_forward(ref.forward_errors(p, v, tri, sqdist, face, bary, lengths), ref.HOST_BOUND_UNITS, "padded")
    assert bool((face[0, 100:] == -1).all()) and bool((face[1] == -1).all()) and bool((face[0, :100] >= 0).all())
    assert bool((dp[0, 100:] == 0).all()) and bool((dp[1] == 0).all()) and bool((dv[1] == 0).all())
    assert float(mean[1]) == 0.0 and bool(torch.isfinite(dv).all())
    # unusable triangles are never chosen; a mesh of them alone gives no result
    mixed = tri.clone()
    mixed[::2, 0] = -1
    mixed[1::4, 2] = V
    face = points.nearest_triangles(p, v, mixed)[1].long()
    usable = ((mixed >= 0) & (mixed < V)).all(dim=1)
    assert bool((face >= 0).all()) and bool(usable[face].all())
    ref.check_forward(ref.forward_errors(p, v, mixed, *points.nearest_triangles(p, v, mixed)), ref.HOST_BOUND_UNITS,
                      "unusable triangles")
    none = torch.full_like(tri, V)
    pl, vl = p.clone().requires_grad_(True), v.clone().requires_grad_(True)
    sqdist, face, bary = points.nearest_triangles(pl, vl, none)
    mean = points.point_mesh_distance(pl, vl, none)
    assert bool((face == -1).all()) and bool((sqdist == 0).all()) and bool((bary == 0).all()) and bool((mean == 0).all())
    (sqdist.sum() + mean.sum()).backward()
    assert bool((pl.grad == 0).all()) and bool((vl.grad == 0).all())
    # NaN and inf in some points and vertices: every face is -1 or a usable triangle
    bad_p, bad_v = p.clone(), v.clone()
    bad_p[0, 5, 1] = float("nan")
    bad_p[1, 9, 0] = float("inf")
    bad_v[0, 7, 2] = float("nan")
    bad_v[1, 11, 0] = float("inf")
    face = points.nearest_triangles(bad_p, bad_v, mixed)[1].long()
    assert int(face[0, 5]) == -1 and int(face[1, 9]) == -1
    assert bool((face >= -1).all()) and bool((face < T).all()) and bool(usable[face[face >= 0]].all())


def test_float64_input_forms_and_chunking(monkeypatch):
    p, v, tri = ref.mesh(4)
    want, want_face = ref.cached_nearest(4)
    sqdist, face, bary = points.nearest_triangles(p.double(), v.double(), tri)
    assert sqdist.dtype == bary.dtype == torch.float64
    agree = face.long() == want_face
    assert float(agree.double().mean()) > 0.99                      # (copies and shared edges tie in real arithmetic)
    assert float((sqdist - want).abs().max()) <= 1e-12
    # a chunk of a few query rows at a time gives the same answer
    whole = points.nearest_triangles(p, v, tri)
    monkeypatch.setattr(points, "_CHUNK_BYTES", 7 * 2 * 1031 * 12 * 4)
    for a, b in zip(whole, points.nearest_triangles(p, v, tri)):
        assert torch.equal(a, b)
    monkeypatch.undo()
    # without the batch axis; int32 and int16 triangles; a non-contiguous view
    one = points.nearest_triangles(p[1], v[1], tri.to(torch.int16))
    assert one[0].shape == (257,) and one[2].shape == (257, 3)
    for a, b in zip(one, whole):
        assert torch.equal(a, b[1])
    assert points.point_mesh_distance(p[1], v[1], tri.to(torch.int32)).dim() == 0
    wide = torch.zeros(2, 257, 6)
    wide[..., 1::2] = p
    for a, b in zip(points.nearest_triangles(wide[..., 1::2], v, tri), whole):
        assert torch.equal(a, b)
    # no gradient wanted: no graph
    assert points.nearest_triangles(p, v, tri)[0].grad_fn is None and points.point_mesh_distance(p, v, tri).grad_fn is None
    vl = v.clone().requires_grad_(True)
    points.point_mesh_distance(p, vl, tri).sum().backward()
    assert p.grad is None and vl.grad is not None


def test_argument_checks():
    p, v, tri = ref.mesh(3)
    with pytest.raises(TypeError):
        points.nearest_triangles(p.numpy(), v, tri)
    with pytest.raises(TypeError):
        points.nearest_triangles(p.long(), v, tri)
    with pytest.raises(TypeError):
        points.nearest_triangles(p, v.long(), tri)
    with pytest.raises(TypeError):
        points.nearest_triangles(p, v, tri.tolist())
    with pytest.raises(RuntimeError):
        points.nearest_triangles(p, v, tri.float())
    with pytest.raises(RuntimeError):
        points.nearest_triangles(p, v.double(), tri)
    with pytest.raises(ValueError):
        points.nearest_triangles(p[..., :2], v, tri)
    with pytest.raises(ValueError):
        points.nearest_triangles(p[0], v, tri)                     # one with, one without the batch axis
    with pytest.raises(ValueError):
        points.nearest_triangles(p[:2], v, tri)
    with pytest.raises(ValueError):
        points.nearest_triangles(p, v, tri[:, :2])
    with pytest.raises(ValueError):
        points.nearest_triangles(p, v, tri[:0])
    with pytest.raises(ValueError):
        points.point_mesh_distance(p, v, tri, lengths=torch.tensor([1, 2]))
    with pytest.raises(RuntimeError):
        points.point_mesh_distance(p, v, tri, lengths=torch.tensor([1.0, 2.0, 3.0]))
    with pytest.raises(TypeError):
        points.point_mesh_distance(p, v, tri, lengths=[1, 2, 3])
    with pytest.raises(RuntimeError):        # the library takes device tensors only
        _native.nearest_triangle_forward(p, v, tri.to(torch.int32))
