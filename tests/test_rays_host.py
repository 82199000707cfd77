"""mesh_renderer.points.cast_rays / rays_occluded on the host: the float32 torch route against the float64 restatement
(tests/ray_reference.py: decided rays name the same face within their bounds, undecided rays name a face float64 does
not reject), known values, watertightness on two closed meshes, the launch plan as a pure function, the analytic
gradient against autograd, and the argument checks.  Nothing here touches a GPU."""
import pytest
import torch

import ray_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes

points = mesh_renderer.points
INF = float("inf")


@pytest.mark.parametrize("name", ref.NAMES)
def test_the_restatement_alone_meets_the_conditions(name):
    decided, easy = ref.shares(ref.truth(name))
    print("%s: decided %.4f, easy %.4f" % (name, decided, easy))
    assert decided >= ref.DECIDED_SHARE and easy >= ref.EASY_SHARE


def test_the_cases_have_hits_and_misses_and_reach_every_launch_shape():
    hits = sum(int((ref.truth(name).face >= 0).sum()) for name in ref.NAMES)
    misses = sum(int(((ref.truth(name).face < 0) & ref.truth(name).decided).sum()) for name in ref.NAMES)
    assert hits > 1000 and misses > 100
    plans = []
    for name in ref.NAMES:
        o, _, _, tri = ref.case(name)
        plans.append(_native.cast_rays_plan(o.shape[0], o.shape[1], tri.shape[0]))
    for lanes in (1, 2):
        assert any(pl["splits"] > 1 and pl["queries_per_lane"] == lanes for pl in plans)
        assert any(pl["splits"] == 1 and pl["queries_per_lane"] == lanes for pl in plans)


@pytest.mark.parametrize("name", ref.NAMES)
def test_torch_route_matches_the_restatement(name):
    o, d, v, tri = ref.case(name)
    t, face, bary = points.cast_rays(o, d, v, tri)
    assert t.dtype == torch.float32 and face.dtype == torch.int32 and bary.dtype == torch.float32
    assert t.shape == o.shape[:2] and face.shape == o.shape[:2] and bary.shape == o.shape
    ref.check(t, face, bary, ref.truth(name), name)
    assert torch.equal(points.rays_occluded(o, d, v, tri), face >= 0)
    one = points.cast_rays(o[0], d[0], v[0], tri.to(torch.int32))   # without the batch axis
    assert one[0].shape == o.shape[1:2] and all(torch.equal(x, y[0]) for x, y in zip(one, (t, face, bary)))


def test_known_values():
    v, tri, _ = shapes.cube(1.0)
    o = torch.tensor([[0.0, 0.0, 2.0]])
    down = torch.tensor([[0.0, 0.0, -1.0]])
    t, face, bary = points.cast_rays(o, down, v, tri)
    assert float(t) == 1.5 and int(face) >= 0 and abs(float(bary.sum()) - 1.0) < 1e-6
    assert torch.allclose(o + t[:, None] * down, torch.tensor([[0.0, 0.0, 0.5]]))
    assert float(points.cast_rays(o, 2 * down, v, tri)[0]) == 0.75          # t is in units of |d|
    far = points.cast_rays(o, down, v, tri, t_min=1.6)
    assert float(far[0]) == 2.5 and int(far[1]) >= 0 and int(far[1]) != int(face)
    t, face, bary = points.cast_rays(o, down, v, tri, t_max=1.0)
    assert float(t) == INF and int(face) == -1 and bool((bary == 0).all())
    assert bool(points.rays_occluded(o, down, v, tri)) and not bool(points.rays_occluded(o, down, v, tri, t_max=1.0))
    assert not bool(points.rays_occluded(o, -down, v, tri))                 # pointing away
    # the line of sight between two points: t_max = 1 along q - p
    p, q = torch.tensor([[2.0, 0.1, 0.2]]), torch.tensor([[-2.0, 0.2, 0.1]])
    assert bool(points.rays_occluded(p, q - p, v, tri, t_max=1.0))
    assert not bool(points.rays_occluded(p, 0.3 * (q - p), v, tri, t_max=1.0))
    # float64 tensors take the same definition
    assert float(points.cast_rays(o.double(), down.double(), v.double(), tri)[0]) == 1.5


def test_plan_is_a_pure_function():
    for name in ref.NAMES:
        o, _, _, tri = ref.case(name)
        plan = _native.cast_rays_plan(o.shape[0], o.shape[1], tri.shape[0])
        assert plan == _native.cast_rays_plan(o.shape[0], o.shape[1], tri.shape[0])
        assert plan == _native.winding_number_plan(o.shape[0], o.shape[1], tri.shape[0])
        assert plan["triangle_tile"] == 128 and plan["workgroup_size"] == 256
        assert 1 <= plan["splits"] <= -(-tri.shape[0] // 128)
    assert _native.cast_rays_plan(1, 512, 100)["queries_per_lane"] == 2
    assert _native.cast_rays_plan(1, 511, 100)["queries_per_lane"] == 1
    assert _native.cast_rays_plan(1, 40, 128)["splits"] == 1
    assert _native.cast_rays_plan(1, 40, 129)["splits"] == 2
    assert _native.cast_rays_plan(1, 10, 1 << 24)["splits"] >= 1
    for bad in ((1, 10, (1 << 24) + 1), (0, 10, 10), (1, 0, 10), (1, 10, 0), (65536, 10, 10)):
        with pytest.raises(ValueError):
            _native.cast_rays_plan(*bad)
    L = _native.lib()
    assert L.mr_cast_rays_workspace_bytes(1, 10, (1 << 24) + 1) == 0
    assert L.mr_cast_rays_workspace_bytes(1, 40, 5000) >= 5000 * 48 + 40 * 40 * 8
    assert L.mr_cast_rays_workspace_bytes(1, 40, 100) >= 100 * 48
    assert L.mr_version() == _native.ABI_VERSION == 356


def test_skipped_and_junk_triangles_change_nothing():
    o, d, v, tri = ref.case("soup_3")
    V = v.shape[1]
    junk = torch.tensor([[0, 1, V], [-1, 2, 3], [4, 4, 5], [6, 7, 6], [8, 8, 8], [2 ** 40, 0, 1]])
    t, face, bary = points.cast_rays(o, d, v, tri)
    mixed = torch.cat([junk, tri[:40], junk, tri[40:], junk])
    t2, face2, bary2 = points.cast_rays(o, d, v, mixed)
    assert torch.equal(t2, t) and torch.equal(bary2, bary)
    moved = torch.where(face < 0, face, face + 6 + 6 * (face >= 40).int())
    assert torch.equal(face2, moved)
    only = points.cast_rays(o, d, v, junk)
    assert bool((only[0] == INF).all()) and bool((only[1] == -1).all()) and bool((only[2] == 0).all())


def test_lengths_equal_the_truncated_call():
    o, d, v, tri = ref.case("soup_3")
    counts = [0, 17, 999]
    out = points.cast_rays(o, d, v, tri, lengths=torch.tensor(counts))
    ref.check(*out, ref.truth_of(o, d, v, tri, torch.tensor(counts)), "lengths", demand_shares=False)
    for b, n in enumerate([0, 17, o.shape[1]]):
        assert bool((out[0][b, n:] == INF).all()) and bool((out[1][b, n:] == -1).all()) and bool((out[2][b, n:] == 0).all())
        if n:
            alone = points.cast_rays(o[b, :n], d[b, :n], v[b], tri)
            assert all(torch.equal(x[b, :n], y) for x, y in zip(out, alone))


def test_non_finite_rays_and_vertices():
    o, d, v, tri = ref.case("soup_7")
    base = points.cast_rays(o, d, v, tri)
    bad_o, bad_d = o.clone(), d.clone()
    bad_o[0, 3, 1] = float("nan")
    bad_o[1, 400, 0] = float("inf")
    bad_d[1, 512, 2] = float("-inf")
    bad_d[0, 7] = 0.0
    bad_d[0, 9, 0] = float("nan")
    out = points.cast_rays(bad_o, bad_d, v, tri)
    dead = torch.zeros(o.shape[:2], dtype=torch.bool)
    dead[0, 3] = dead[1, 400] = dead[1, 512] = dead[0, 7] = dead[0, 9] = True
    assert bool((out[0][dead] == INF).all()) and bool((out[1][dead] == -1).all()) and bool((out[2][dead] == 0).all())
    assert all(torch.equal(x[~dead], y[~dead]) for x, y in zip(out, base))
    # a NaN vertex takes its triangles out of image 1 and leaves image 0 alone
    hit = int(base[1][1, 0])
    assert hit >= 0
    bad_v = v.clone()
    bad_v[1, int(tri[hit, 0])] = float("nan")
    out = points.cast_rays(o, d, bad_v, tri)
    assert all(torch.equal(x[0], y[0]) for x, y in zip(out, base))
    gone = (tri == tri[hit, 0]).any(dim=1)
    assert not bool(gone[out[1][1].clamp(min=0).long()][out[1][1] >= 0].any())
    assert not bool(torch.isnan(out[0]).any()) and not bool(torch.isnan(out[2]).any())
    ref.check(*out, ref.truth_of(o, d, bad_v, tri), "a NaN vertex", demand_shares=False)


def test_watertightness():
    ref.check_watertight(points.cast_rays)


def test_analytic_gradient_against_autograd():
    for name in ("soup_3", "cube", "sphere_translated"):
        o, d, v, tri = ref.case(name)
        og, dg, vg = (x.double().clone().requires_grad_(True) for x in (o, d, v))
        t, face, bary = points.cast_rays(og, dg, vg, tri)
        assert t.requires_grad and not face.requires_grad and not bary.requires_grad
        w = torch.randn(t.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(21))
        torch.where(face >= 0, t, torch.zeros_like(t)).mul(w).sum().backward()
        want = ref.gradients(o, d, v, tri, face, w)
        for got, ref_grad, what in zip((og.grad, dg.grad, vg.grad), want, ("origins", "directions", "vertices")):
            scale = float(ref_grad.abs().max())
            err = float((got - ref_grad).abs().max())
            print("%s d%s: max err %.3g of scale %.3g" % (name, what, err, scale))
            assert scale > 0 and err <= 1e-9 * scale
        miss = face < 0
        assert bool(miss.any()) or name != "soup_3"
        assert bool((og.grad[miss] == 0).all()) and bool((dg.grad[miss] == 0).all())


def test_gradients_only_where_required_and_never_nan():
    o, d, v, tri = ref.case("soup_3")
    lengths = torch.tensor([65, 20, 0])
    og = o.clone().requires_grad_(True)
    t, face, _ = points.cast_rays(og, d, v, tri, lengths=lengths)
    assert bool((face[1, 20:] == -1).all()) and bool((face[2] == -1).all())
    t.backward(torch.where(face >= 0, 1.0, float("nan")))   # a NaN upstream of a miss: the gradient is still exactly 0
    assert bool((og.grad[face < 0] == 0).all()) and bool(torch.isfinite(og.grad).all())
    vg = v.clone().requires_grad_(True)
    t, face, _ = points.cast_rays(o, d, vg, tri, lengths=lengths)
    torch.where(face >= 0, t, torch.zeros_like(t)).sum().backward()
    assert bool(torch.isfinite(vg.grad).all()) and float(vg.grad.abs().max()) > 0
    assert not points.cast_rays(o, d, v, tri)[0].requires_grad
    # a ray in the plane of its triangle never hits it; one that grazes keeps a finite gradient or none
    flat_v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], requires_grad=True)
    flat = points.cast_rays(torch.tensor([[-1.0, 0.2, 0.0]]), torch.tensor([[1.0, 0.0, 0.0]]), flat_v, torch.tensor([[0, 1, 2]]))
    assert int(flat[1]) == -1


def test_argument_errors():
    o, d, v, tri = ref.case("soup_3")
    for fn in (points.cast_rays, points.rays_occluded):
        with pytest.raises(TypeError):
            fn(o.numpy(), d, v, tri)
        with pytest.raises(TypeError):
            fn(o, d.long(), v, tri)
        with pytest.raises(TypeError):
            fn(o, d, v, tri.tolist())
        with pytest.raises((TypeError, RuntimeError)):
            fn(o, d, v, tri.float())
        with pytest.raises(RuntimeError):
            fn(o, d, v.double(), tri)
        with pytest.raises(RuntimeError):
            fn(o, d.double(), v, tri)
        with pytest.raises(ValueError):
            fn(o[..., :2], d[..., :2], v, tri)
        with pytest.raises(ValueError):
            fn(o, d[:, :5], v, tri)
        with pytest.raises(ValueError):
            fn(o[0], d[0], v, tri)
        with pytest.raises(ValueError):
            fn(o[:2], d[:2], v, tri)
        with pytest.raises(ValueError):
            fn(o, d, v, tri[:, :2])
        with pytest.raises(ValueError):
            fn(o, d, v, tri, lengths=torch.tensor([1, 2]))
        with pytest.raises(RuntimeError):
            fn(o, d, v, tri, lengths=torch.tensor([1.0, 2.0, 3.0]))
        for t_min, t_max in ((-0.1, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("nan")), ("0", 1.0)):
            with pytest.raises(ValueError):
                fn(o, d, v, tri, t_min=t_min, t_max=t_max)
    with pytest.raises(RuntimeError):   # the native wrapper is HIP only
        _native.cast_rays_forward(o, d, v, tri.to(torch.int32))
