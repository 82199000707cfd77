"""mesh_renderer.points.winding_number / inside_mesh / signed_distance on the host: the float32 torch route against the
float64 restatement (tests/winding_reference.py: every query within its own rounding bound E_i), the launch plan as a
pure function, and the argument checks.  Nothing here touches a GPU."""
import pytest
import torch

import winding_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes

points = mesh_renderer.points


@pytest.mark.parametrize("name", ref.NAMES)
def test_torch_route_matches_the_restatement(name):
    p, v, tri = ref.case(name)
    want, bound = ref.truth(name)
    w = points.winding_number(p, v, tri)
    assert w.dtype == torch.float32 and w.shape == p.shape[:2] and not w.requires_grad
    ref.check(w, want, bound, name)


def test_known_values():
    v, tri, _ = shapes.cube(1.0)
    assert float(points.winding_number(torch.zeros(1, 3), v, tri)) == 1.0
    assert abs(float(points.winding_number(torch.tensor([[2.0, 0.1, 0.3]]), v, tri))) < 1e-6
    flipped = torch.flip(tri, [1])
    assert float(points.winding_number(torch.zeros(1, 3), v, flipped)) == -1.0
    want, bound = ref.truth("sphere")
    assert abs(float(want[0, 0]) - 0.96) < 1e-3     # the package's sphere is not watertight
    p, sv, st = ref.case("sphere")
    assert abs(float(points.winding_number(p[0, :1], sv[0], st)) - float(want[0, 0])) <= float(bound[0, 0])


def test_plan_is_a_pure_function():
    plans = {}
    for name in ref.NAMES:
        p, _, tri = ref.case(name)
        plans[name] = _native.winding_number_plan(p.shape[0], p.shape[1], tri.shape[0])
        assert plans[name] == _native.winding_number_plan(p.shape[0], p.shape[1], tri.shape[0])
        assert plans[name]["splits"] >= 1 and plans[name]["queries_per_lane"] in (1, 2)
        assert plans[name]["triangle_tile"] == 128 and plans[name]["workgroup_size"] == 256
        tiles = -(-tri.shape[0] // plans[name]["triangle_tile"])
        assert plans[name]["splits"] <= tiles
    # both routes of the sum, both kernels, and the thresholds the cases straddle
    assert any(pl["splits"] > 1 for pl in plans.values()) and any(pl["splits"] == 1 for pl in plans.values())
    assert {pl["queries_per_lane"] for pl in plans.values()} == {1, 2}
    assert any(pl["splits"] > 1 and pl["queries_per_lane"] == 2 for pl in plans.values())
    assert any(pl["splits"] == 1 and pl["queries_per_lane"] == 2 for pl in plans.values())
    assert _native.winding_number_plan(1, 512, 100)["queries_per_lane"] == 2
    assert _native.winding_number_plan(1, 511, 100)["queries_per_lane"] == 1
    assert _native.winding_number_plan(1, 40, 128)["splits"] == 1
    assert _native.winding_number_plan(1, 40, 129)["splits"] == 2
    assert _native.winding_number_plan(1, 10, 1 << 24)["splits"] >= 1
    for bad in ((1, 10, (1 << 24) + 1), (0, 10, 10), (1, 0, 10), (1, 10, 0), (65536, 10, 10)):
        with pytest.raises(ValueError):
            _native.winding_number_plan(*bad)
    assert _native.lib().mr_winding_number_workspace_bytes(1, 10, (1 << 24) + 1) == 0
    assert _native.lib().mr_winding_number_workspace_bytes(1, 40, 5000) >= 5000 * 48 + 40 * 40 * 8
    assert _native.lib().mr_version() == _native.ABI_VERSION == 356


def test_permuted_skipped_and_padded_triangles():
    """On the host the sum is exact but torch's vectorised kernels may round a TERM differently depending on where it
    sits in memory, so these hold within the bound here and bit for bit on the GPU (tests/test_winding_gpu.py)."""
    p, v, tri = ref.case("soup_3")
    want, bound = ref.truth("soup_3")
    perm = torch.randperm(tri.shape[0], generator=torch.Generator().manual_seed(5))
    ref.check(points.winding_number(p, v, tri[perm]), want, bound, "permuted")
    V = v.shape[1]
    junk = torch.tensor([[0, 1, V], [-1, 2, 3], [4, 4, 5], [6, 7, 6], [8, 8, 8]])
    padded_bound = bound + 10 * 2.0 ** -41   # T counts the skipped triangles too
    ref.check(points.winding_number(p, v, torch.cat([junk, tri, junk])), want, padded_bound, "with skipped triangles")
    for b in range(p.shape[0]):
        ref.check(points.winding_number(p[b], v[b], tri)[None], want[b:b + 1], bound[b:b + 1], "image %d alone" % b)
    lengths = torch.tensor([0, 17, 999])
    out = points.winding_number(p, v, tri, lengths)
    want, bound = ref.winding(p, v, tri, lengths)
    ref.check(out, want, bound, "lengths")
    for b, n in enumerate([0, 17, 65]):
        assert bool((out[b, n:] == 0).all()) and (n == 0 or bool((out[b, :n] != 0).any()))


def test_non_finite_input():
    p, v, tri = ref.case("soup_7")
    base = points.winding_number(p, v, tri)
    bad = p.clone()
    bad[0, 3, 1] = float("nan")
    bad[1, 400, 0] = float("inf")
    w = points.winding_number(bad, v, tri)
    hit = torch.zeros_like(base, dtype=torch.bool)
    hit[0, 3] = hit[1, 400] = True
    assert bool(torch.isnan(w[hit]).all()) and torch.allclose(w[~hit], base[~hit], rtol=0, atol=1e-5)
    bad_v = v.clone()
    bad_v[1, int(tri[0, 0])] = float("nan")
    w = points.winding_number(p, bad_v, tri, torch.tensor([513, 100]))
    assert torch.allclose(w[0], base[0], rtol=0, atol=1e-5)
    assert bool(torch.isnan(w[1, :100]).all()) and bool((w[1, 100:] == 0).all())
    assert not bool(points.inside_mesh(p, bad_v, tri)[1].any())


def test_inside_mesh_and_signed_distance_on_the_host():
    p, v, tri = ref.case("cube")
    exact = ref.box_signed_distance(p)
    clear = exact.abs() >= 0.01
    inside = points.inside_mesh(p, v, tri)
    assert inside.dtype == torch.bool and inside.shape == p.shape[:2]
    assert torch.equal(inside[clear], (p.abs().max(-1).values < 0.5)[clear]) and bool(inside.any()) and not bool(inside.all())
    assert not bool(points.inside_mesh(p, v, tri, torch.tensor([300, 7]))[1, 7:].any())
    assert not bool(points.inside_mesh(p, v, tri, threshold=1.5).any())
    pg, vg = p.clone().requires_grad_(True), v.clone().requires_grad_(True)
    sd = points.signed_distance(pg, vg, tri)
    assert sd.dtype == torch.float32 and sd.shape == p.shape[:2]
    assert torch.equal(sd.detach().abs(), points.nearest_triangles(p, v, tri)[0].sqrt())
    assert bool(((sd.detach() < 0) == (exact < 0))[clear].all())
    assert float((sd.detach().double() - exact).abs().max()) < 1e-5
    sd.sum().backward()
    assert bool(torch.isfinite(pg.grad).all()) and bool(torch.isfinite(vg.grad).all())
    # the gradient to a point is the unit direction away from the surface, on either side of it
    assert float((pg.grad.norm(dim=-1) - 1).abs().max()) < 1e-4
    # a query on a vertex of the cube: distance 0, gradient 0 (not NaN)
    on = v[:1, 3:4].clone().requires_grad_(True)
    sd = points.signed_distance(on, v[:1], tri)
    sd.sum().backward()
    assert float(sd.detach()) == 0.0 and bool((on.grad == 0).all())
    # one image without the batch axis
    assert torch.allclose(points.signed_distance(p[1], v[1], tri), points.signed_distance(p, v, tri)[1], atol=1e-6)


def test_argument_errors():
    p, v, tri = ref.case("soup_3")
    for fn in (points.winding_number, points.inside_mesh, points.signed_distance):
        with pytest.raises(TypeError):
            fn(p.numpy(), v, tri)
        with pytest.raises(TypeError):
            fn(p.long(), v, tri)
        with pytest.raises(TypeError):
            fn(p, v, tri.tolist())
        with pytest.raises((TypeError, RuntimeError)):
            fn(p, v, tri.float())
        with pytest.raises(RuntimeError):
            fn(p, v.double(), tri)
        with pytest.raises(ValueError):
            fn(p[..., :2], v, tri)
        with pytest.raises(ValueError):
            fn(p[0], v, tri)
        with pytest.raises(ValueError):
            fn(p[:2], v, tri)
        with pytest.raises(ValueError):
            fn(p, v, tri[:, :2])
        with pytest.raises(ValueError):
            fn(p, v, tri, lengths=torch.tensor([1, 2]))
        with pytest.raises(RuntimeError):
            fn(p, v, tri, lengths=torch.tensor([1.0, 2.0, 3.0]))
    with pytest.raises(RuntimeError):   # the native wrapper is HIP only
        _native.winding_number_forward(p, v, tri.to(torch.int32))
    for name in ("winding_number", "inside_mesh", "signed_distance"):
        assert callable(getattr(mesh_renderer.points, name))
