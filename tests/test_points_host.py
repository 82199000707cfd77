"""mesh_renderer.points on the host: the chunked torch path of nearest_points / chamfer_distance and the surface
sampler against the float64 restatement (tests/points_reference.py), the argument checks and the launch plan.

Budgets (the GPU tests' too): sqdist within 1e-6 relative of float64 -- the difference form costs one rounding each
in the subtraction, the product and the two sums, below 4 * 2^-24; Chamfer values within 1e-5 relative (a reordered
float32 sum); gradients within 1e-4 of the largest magnitude of the expected gradient tensor."""
import ctypes

import numpy as np
import pytest
import torch

import points_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes

points = mesh_renderer.points
ALL_CLOUDS = list(range(len(ref.SHAPES))) + ["translated"]


def _clouds(k):
    return ref.translated_clouds() if k == "translated" else ref.clouds(k)


def test_the_module_is_exported():
    assert mesh_renderer.points.chamfer_distance is points.chamfer_distance
    for name in ("nearest_points", "chamfer_distance", "sample_surface_points", "sample_surface_points_from_uniforms"):
        assert callable(getattr(points, name))


@pytest.mark.parametrize("k", list(range(len(ref.SHAPES))))
def test_the_reference_has_no_ambiguous_neighbours(k):
    """What the GPU tests' index equality relies on: on every seeded shape, in both directions, the runner-up is
    further than 4e-6 relative from the nearest point."""
    for reverse in (False, True):
        _, _, gap = ref.cached_nearest(k, reverse)
        assert int((gap <= ref.RUNNER_UP_MARGIN).sum()) == 0


@pytest.mark.parametrize("k", ALL_CLOUDS)
def test_torch_path_matches_the_restatement(k):
    x, y = _clouds(k)
    want, want_idx, gap = ref.nearest(x, y)
    xl, yl = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    got, idx = points.nearest_points(xl, yl)
    assert got.dtype == torch.float32 and idx.dtype == torch.int32 and got.shape == idx.shape == x.shape[:2]
    assert not idx.requires_grad
    assert bool(((got.detach().double() - want).abs() <= 1e-6 * want).all())
    near = ref.distance_to(x, y, idx)
    assert bool(((near - want).abs() <= 1e-6 * want).all())
    clear = gap > ref.RUNNER_UP_MARGIN
    assert int((~clear).sum()) <= 0.01 * clear.numel() and torch.equal(idx.long()[clear], want_idx[clear])
    g = torch.Generator().manual_seed(3)
    upstream = torch.randn(got.shape, generator=g)
    got.backward(upstream)
    wdx, wdy = ref.nearest_gradients(x, y, idx, upstream)
    assert float((xl.grad.double() - wdx).abs().max()) <= 1e-4 * float(wdx.abs().max())
    assert float((yl.grad.double() - wdy).abs().max()) <= 1e-4 * float(wdy.abs().max())
    # Chamfer, both directions
    xl, yl = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    total = points.chamfer_distance(xl, yl, x_weight=0.75, y_weight=1.5)
    want_total = ref.chamfer(x, y, x_weight=0.75, y_weight=1.5)
    assert total.shape == (x.shape[0],)
    assert bool(((total.detach().double() - want_total).abs() <= 1e-5 * want_total).all())
    weights = torch.randn(x.shape[0], generator=g)
    total.backward(weights)
    wdx, wdy = ref.chamfer_gradients(x, y, idx, points.nearest_points(y, x)[1], weights, x_weight=0.75, y_weight=1.5)
    assert float((xl.grad.double() - wdx).abs().max()) <= 1e-4 * float(wdx.abs().max())
    assert float((yl.grad.double() - wdy).abs().max()) <= 1e-4 * float(wdy.abs().max())


def test_float64_clouds_and_chunking(monkeypatch):
    x, y = ref.clouds(4)
    want, want_idx, _ = ref.nearest(x, y)
    got, idx = points.nearest_points(x.double(), y.double())
    assert got.dtype == torch.float64 and torch.equal(idx.long(), want_idx)
    assert float((got - want).abs().max()) <= 1e-12
    # a chunk of a few query rows at a time gives the same answer
    monkeypatch.setattr(points, "_CHUNK_BYTES", 7 * 2 * 1031 * 3 * 4)
    chunked, chunked_idx = points.nearest_points(x, y)
    whole, whole_idx = ref.nearest(x, y)[:2]
    assert torch.equal(chunked_idx.long(), whole_idx)
    assert bool(((chunked.double() - whole).abs() <= 1e-6 * whole).all())


def test_ties_go_to_the_lowest_index():
    for wide in (False, True):
        x, y = ref.lattice_clouds(wide)
        want, want_idx, _ = ref.nearest(x, y)
        got, idx = points.nearest_points(x, y)
        assert bool((want == 0.75).all()) and torch.equal(got.double(), want)
        assert torch.equal(idx.long(), want_idx)


def test_unbatched_forms():
    x, y = ref.clouds(3)
    d, i = points.nearest_points(x[1], y[1])
    db, ib = points.nearest_points(x[1:2], y[1:2])
    assert d.shape == (65,) and i.shape == (65,) and torch.equal(d, db[0]) and torch.equal(i, ib[0])
    c = points.chamfer_distance(x[1], y[1])
    assert c.dim() == 0 and float(c) == float(points.chamfer_distance(x[1:2], y[1:2])[0])
    d, _ = points.nearest_points(x[1], y[1], y_lengths=torch.tensor([10]))
    assert torch.equal(d, points.nearest_points(x[1], y[1, :10])[0])


def test_lengths():
    x, y = ref.clouds(3)           # (3, 65, 63)
    x, y = x.clone(), y.clone()
    xl, yl = torch.tensor([65, 0, 20]), torch.tensor([10, 63, 0])
    for b in range(3):             # what lies beyond the lengths must not matter
        x[b, int(xl[b]):] = 1e30
        y[b, int(yl[b]):] = 1e30
    want, want_idx, _ = ref.nearest(x, y, xl, yl)
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    got, idx = points.nearest_points(xg, yg, xl, yl)
    assert torch.equal(idx.long(), want_idx)
    assert bool(((got.detach().double() - want).abs() <= 1e-6 * want).all())
    assert bool((idx[1] == -1).all()) and bool((idx[2] == -1).all()) and bool((got[1:] == 0).all())
    assert bool((idx[0] >= 0).all()) and bool((idx[0] < 10).all())
    got.sum().backward()
    assert bool(torch.isfinite(xg.grad).all()) and bool(torch.isfinite(yg.grad).all())
    assert bool((xg.grad[1:] == 0).all()) and bool((yg.grad[1:] == 0).all()) and bool((yg.grad[0, 10:] == 0).all())
    total = points.chamfer_distance(x, y, xl, yl)
    want_total = ref.chamfer(x, y, xl, yl)
    assert float(total[1]) == 0.0 and float(total[2]) == 0.0 and float(want_total[1]) == 0.0
    assert abs(float(total[0]) - float(want_total[0])) <= 1e-5 * float(want_total[0])
    # lengths above the cloud and below zero are clamped; int32 and int64 agree
    over = points.nearest_points(x, y, torch.tensor([1000, 65, 66]), torch.tensor([64, 63, 10 ** 6], dtype=torch.int64))
    plain = points.nearest_points(x, y)
    assert torch.equal(over[0], plain[0]) and torch.equal(over[1], plain[1])
    under = points.nearest_points(x, y, torch.tensor([-5, 65, 65], dtype=torch.int32), None)
    assert bool((under[1][0] == -1).all()) and torch.equal(under[1][1:], plain[1][1:])


def test_a_zero_weight_gives_the_other_direction_alone():
    x, y = ref.clouds(6)
    both = ref.chamfer(x, y)
    one = points.chamfer_distance(x, y, x_weight=0.0)
    other = points.chamfer_distance(x, y, y_weight=0)
    want_yx = ref.chamfer(x, y, x_weight=0.0)
    assert bool(((one.double() - want_yx).abs() <= 1e-5 * want_yx).all())
    assert bool(((one.double() + other.double() - both).abs() <= 1e-5 * both).all())
    assert bool((points.chamfer_distance(x, y, x_weight=0.0, y_weight=0.0) == 0).all())


def test_argument_errors():
    x, y = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    for fn in (points.nearest_points, points.chamfer_distance):
        with pytest.raises(TypeError):
            fn([0.0, 0.0, 0.0], y)
        with pytest.raises(TypeError):
            fn(x, y.long())
        with pytest.raises(ValueError):
            fn(x[..., :2], y)
        with pytest.raises(ValueError):
            fn(x, torch.zeros(3, 7, 3))
        with pytest.raises(ValueError):
            fn(x[0], y)
        with pytest.raises(ValueError):
            fn(x, torch.zeros(2, 0, 3))
        with pytest.raises(RuntimeError):
            fn(x, y.double())
        with pytest.raises(RuntimeError):
            fn(x, y, x_lengths=torch.tensor([1.0, 2.0]))
        with pytest.raises(ValueError):
            fn(x, y, y_lengths=torch.tensor([1, 2, 3]))
        with pytest.raises(TypeError):
            fn(x, y, x_lengths=[1, 2])
    tri = torch.tensor([[0, 1, 2]])
    v = torch.eye(3)
    with pytest.raises(RuntimeError, match="integer vertex indices"):
        points.sample_surface_points(v, tri.float(), 4)
    with pytest.raises(TypeError):
        points.sample_surface_points(v.long(), tri, 4)
    with pytest.raises(ValueError):
        points.sample_surface_points(v[:, :2], tri, 4)
    with pytest.raises(ValueError):
        points.sample_surface_points(v, tri[:, :2], 4)
    with pytest.raises(ValueError):
        points.sample_surface_points(v, tri, 0)
    with pytest.raises(ValueError):
        points.sample_surface_points_from_uniforms(v[None], tri, torch.zeros(2, 4, 3))
    with pytest.raises(ValueError, match="total area 0"):
        points.sample_surface_points(torch.ones(3, 3), tri, 4)
    with pytest.raises(ValueError, match="total area 0"):   # one image of the batch is enough
        points.sample_surface_points(torch.stack([v, torch.zeros(3, 3)]), tri, 4)


def test_nearest_plan_is_sane():
    for shape in ref.SHAPES + [(8, 10000, 10000), (32, 2502, 20000), (1, 100000, 100000), (65535, 1, 1)]:
        plan = _native.nearest_plan(*shape)
        assert plan["splits"] >= 1 and plan["queries_per_lane"] >= 1 and plan["target_tile"] >= 1
        assert plan["splits"] <= -(-shape[2] // plan["target_tile"])
    assert _native.nearest_plan(1, 4096, 64)["splits"] == 1
    assert _native.nearest_plan(1, 40, 5000)["splits"] > 1
    with pytest.raises(ValueError):
        _native.nearest_plan(0, 4, 4)
    with pytest.raises(ValueError):
        _native.nearest_plan(1, 4, (1 << 28) + 1)


def test_abi_validates_before_touching_a_device():
    L = _native.lib()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)   # never dereferenced: the calls below are rejected first
    assert L.mr_nearest_workspace_bytes(0, 4, 4) == 0 and L.mr_nearest_workspace_bytes(1, 4, 0) == 0
    assert L.mr_nearest_workspace_bytes(1, 4, 4) >= 256
    assert L.mr_nearest_forward(null, null, null, null, 1, 4, 4, null, null, null, 1.0, 0, null, 0, null) == _native.MR_EINVAL
    assert L.mr_nearest_forward(one, one, null, null, 1, 4, 4, null, one, null, 1.0, 0, null, 0, null) == _native.MR_EWORKSPACE
    assert L.mr_nearest_forward(one, one, null, null, 70000, 4, 4, null, one, null, 1.0, 0, one, 4096, null) == _native.MR_EINVAL
    backward = lambda *a: L.mr_nearest_backward(one, one, null, null, 1, 4, 4, *a, 1.0, 1.0, one, one, null)
    assert backward(null, null, null, null, null, null, null, one) == _native.MR_EINVAL        # no direction
    assert backward(one, one, one, null, null, null, one, one) == _native.MR_EINVAL            # two upstreams
    assert backward(one, null, null, null, null, null, null, one) == _native.MR_EINVAL         # dy without its index
    assert backward(one, one, one, one, one, one, one, null) == _native.MR_EINVAL              # per point, two directions
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.nearest_forward(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))


def _mesh_with_a_zero_area_face():
    vertices = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.5], [2.0, 0.0, 0.0]])
    # face 1 is a segment (0, 1, 4 are collinear), and so is the last face
    triangles = torch.tensor([[0, 1, 2], [0, 1, 4], [1, 3, 2], [1, 4, 3], [0, 4, 1]], dtype=torch.int32)
    return vertices, triangles


def test_sampling_matches_the_restatement():
    vertices, triangles = _mesh_with_a_zero_area_face()
    g = torch.Generator().manual_seed(5)
    uniforms = torch.rand(200, 3, generator=g)
    want, want_faces, want_bary = ref.sample(vertices, triangles, uniforms)
    got, faces, bary = points.sample_surface_points_from_uniforms(vertices, triangles, uniforms, return_faces=True)
    assert got.shape == (200, 3) and faces.shape == (200,) and bary.shape == (200, 3)
    assert torch.equal(faces, want_faces)
    assert float((bary.double() - want_bary).abs().max()) <= 1e-6
    assert float((got.double() - want).abs().max()) <= 1e-6
    # batched, a second image scaled: the same faces (areas scale together), scaled points
    batch = torch.stack([vertices, 3.0 * vertices])
    both = points.sample_surface_points_from_uniforms(batch, triangles.long(), torch.stack([uniforms, uniforms]))
    assert torch.equal(both[0], got) and float((both[1] - 3.0 * got).abs().max()) <= 1e-5


def test_sampled_barycentrics_and_the_zero_area_face():
    vertices, triangles = _mesh_with_a_zero_area_face()
    g = torch.Generator().manual_seed(6)
    got, faces, bary = points.sample_surface_points(vertices, triangles, 20000, generator=g, return_faces=True)
    assert got.shape == (20000, 3)
    assert bool((bary >= 0).all()) and float((bary.sum(-1) - 1.0).abs().max()) <= 1e-6
    corners = vertices[triangles.long()[faces]]
    assert float((got - (bary[..., None] * corners).sum(1)).abs().max()) <= 1e-6
    assert set(faces.tolist()) == {0, 2, 3}
    # the ends of the unit interval
    edge = torch.tensor([[0.0, 0.0, 0.0], [1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24], [1.0, 1.0, 1.0]])
    _, faces, _ = points.sample_surface_points_from_uniforms(vertices, triangles, edge, return_faces=True)
    assert faces.tolist() == [0, 3, 3]
    # seeded: the same generator state gives the same points
    a = points.sample_surface_points(vertices, triangles, 16, generator=torch.Generator().manual_seed(1))
    b = points.sample_surface_points(vertices, triangles, 16, generator=torch.Generator().manual_seed(1))
    assert torch.equal(a, b)


def test_sampling_is_area_weighted_on_the_cube():
    vertices, triangles, _ = shapes.cube(2.0)
    assert triangles.shape == (12, 3)
    g = torch.Generator().manual_seed(0)
    _, faces, _ = points.sample_surface_points(vertices, triangles, 24000, generator=g, return_faces=True)
    counts = torch.bincount(faces, minlength=12)
    sigma = (24000 * (1 / 12) * (11 / 12)) ** 0.5
    assert 42 < sigma < 44 and int(counts.sum()) == 24000
    assert float((counts.double() - 2000).abs().max()) <= 6 * sigma, counts.tolist()


def test_sampled_points_gradient():
    vertices, triangles = _mesh_with_a_zero_area_face()
    g = torch.Generator().manual_seed(8)
    uniforms = torch.rand(2, 9, 3, generator=g, dtype=torch.float64)
    batch = torch.stack([vertices, vertices * 1.5 + 0.1]).double().requires_grad_(True)
    fn = lambda v: points.sample_surface_points_from_uniforms(v, triangles, uniforms)
    assert torch.autograd.gradcheck(fn, (batch,))
    # the face choice carries no gradient: the points are linear in the vertices
    out, faces, bary = points.sample_surface_points_from_uniforms(batch, triangles, uniforms, return_faces=True)
    assert out.requires_grad and not faces.requires_grad and not bary.requires_grad
