"""mesh_renderer.points.triangle_nearest_points / mesh_point_distance / point_mesh_face_distance on the host: the
chunked torch path against the float64 restatement (tests/mesh_point_reference.py), the launch plan's invariants,
the C ABI's argument checks and the Python ones.

Forward bound: mp.HOST_BOUND_UNITS (twice the torch path's own measured worst, 2.25) in units of 2^-24 * scale,
scale = max_k |p_j - v_k|^2 over the corners of the named pair; an index equals the restatement's wherever its
minimum is separated from the runner-up by more than that bound; gradients within 1e-4 of the largest magnitude of
the expected gradient tensor, the restatement being evaluated with the returned (index, bary)."""
import ctypes

import pytest
import torch

import mesh_point_reference as mp
import point_mesh_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer

points = mesh_renderer.points


def _grad_close(got, want, what):
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    print("%s: gradient max err %.3g of scale %.3g" % (what, err, scale))
    assert err <= 1e-4 * scale, "%s: gradient error %.3g > 1e-4 * %.3g" % (what, err, scale)


def test_the_functions_are_exported():
    for name in ("triangle_nearest_points", "mesh_point_distance", "point_mesh_face_distance"):
        assert callable(getattr(mesh_renderer.points, name))


def test_the_measured_worst_is_the_one_written_down():
    assert mp.HOST_WORST_UNITS == 2.25 and mp.HOST_WORST_CASE in mp.CASES
    assert mp.HOST_BOUND_UNITS == 4.5 and mp.HIP_BOUND_UNITS == 9.0


def test_the_shapes_cover_every_launch_path():
    plan = lambda shape: _native.nearest_point_of_triangle_plan(shape[0], shape[1], shape[3])
    own = [plan(s) for s in mp.SHAPES]
    for p in own:
        assert p["point_tile"] == 256 and p["workgroup_size"] == 256
    assert own[0]["splits"] == 2 and own[0]["points_per_step"] == 2 and mp.SHAPES[0][1] == own[0]["point_tile"] + 1
    assert own[1]["splits"] == 3 and mp.SHAPES[1][1] == 5 * own[1]["point_tile"] + 1     # two tiles a split, one lone
    assert mp.SHAPES[2][3] == own[2]["workgroup_size"] + 1
    assert own[3]["splits"] == 9 and own[3]["points_per_step"] == 2
    assert own[4]["splits"] == 1 and own[4]["points_per_step"] == 2
    assert own[5]["splits"] == 1 and own[5]["points_per_step"] == 1
    assert mp.SHAPES[3][2:] == mp.SHAPES[4][2:] == mp.SHAPES[5][2:]
    assert _native.nearest_point_of_triangle_plan(1, 255, 100)["points_per_step"] == 1
    assert _native.nearest_point_of_triangle_plan(1, 256, 100)["points_per_step"] == 2
    # a small mesh against a large cloud fills the chip
    assert _native.nearest_point_of_triangle_plan(1, 100000, 200)["splits"] == 391


def test_the_plan_covers_every_point_once_and_refuses_sizes_outside_the_limits():
    for B in (1, 2, 7, 32, 5000):
        for N in (1, 255, 256, 257, 511, 512, 513, 20000, 100000):
            for T in (1, 200, 255, 256, 257, 5000, 49928):
                p = _native.nearest_point_of_triangle_plan(B, N, T)
                tile = p["point_tile"]
                tiles = -(-N // tile)
                chunk = -(-tiles // p["splits"]) * tile            # points per split: whole tiles
                assert 1 <= p["splits"] <= tiles
                assert (p["splits"] - 1) * chunk < N                # the last split still has a point
                assert p["splits"] * chunk >= N                     # disjoint runs [s chunk, (s + 1) chunk) cover N
                assert p["points_per_step"] == (2 if N >= 256 else 1)
    for bad in ((0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, 1, 0), (1, (1 << 28) + 1, 1), (1, 1, (1 << 28) + 1),
                (65535, 1 << 21, 1), (65535, 1, 1 << 21), (-1, 5, 5)):
        with pytest.raises(ValueError):
            _native.nearest_point_of_triangle_plan(*bad)
    big = _native.nearest_point_of_triangle_plan(1, 1 << 28, 1 << 28)
    assert 1 <= big["splits"] <= (1 << 20)
    assert _native.lib().mr_nearest_point_of_triangle_workspace_bytes(1, 1 << 28, 1 << 28) > (80 << 28)


def test_the_abi_refuses_null_pointers_and_bad_sizes():
    L = _native.lib()
    EINVAL, EWORKSPACE = _native.MR_EINVAL, _native.MR_EWORKSPACE
    out = (ctypes.c_int * 4)()
    slot = lambda k: ctypes.c_void_p(ctypes.addressof(out) + 4 * k)
    assert L.mr_nearest_point_of_triangle_plan(1, 10, 10, slot(0), slot(1), slot(2), slot(3)) == _native.MR_OK
    for missing in range(4):
        args = [None if k == missing else slot(k) for k in range(4)]
        assert L.mr_nearest_point_of_triangle_plan(1, 10, 10, *args) == EINVAL
    assert L.mr_nearest_point_of_triangle_plan(0, 10, 10, slot(0), slot(1), slot(2), slot(3)) == EINVAL
    assert L.mr_nearest_point_of_triangle_workspace_bytes(1, 0, 10) == 0
    assert L.mr_nearest_point_of_triangle_workspace_bytes(1, 10, -1) == 0
    need = L.mr_nearest_point_of_triangle_workspace_bytes(2, 10, 10)
    assert need >= 2 * 10 * 80
    # host buffers stand in for device pointers: every call below is refused before anything is launched
    buf = ctypes.create_string_buffer(1 << 16)
    a = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    fwd = lambda **kw: L.mr_nearest_point_of_triangle_forward(*[kw.get(k, d) for k, d in (
        ("points", a), ("vertices", a), ("triangles", a), ("lengths", None), ("B", 2), ("N", 10), ("V", 10), ("T", 10),
        ("sqdist", a), ("index", a), ("bary", a), ("total", None), ("usable", None), ("ws", a), ("ws_bytes", need),
        ("stream", None))])
    for name in ("points", "vertices", "triangles", "index", "bary"):
        assert fwd(**{name: None}) == EINVAL, name
    assert fwd(total=a) == EINVAL                          # the mean needs the count's slot
    assert fwd(ws=None) == EWORKSPACE and fwd(ws_bytes=need - 1) == EWORKSPACE
    assert fwd(ws=ctypes.c_void_p(a.value + 16)) == EWORKSPACE   # 256-byte aligned, as every workspace
    for name, value in (("B", 0), ("B", 65536), ("N", 0), ("V", 0), ("T", 0), ("N", (1 << 28) + 1), ("V", -3)):
        assert fwd(**{name: value}) == EINVAL, (name, value)
    bwd = lambda **kw: L.mr_nearest_point_of_triangle_backward(*[kw.get(k, d) for k, d in (
        ("points", a), ("vertices", a), ("triangles", a), ("lengths", None), ("B", 2), ("N", 10), ("V", 10), ("T", 10),
        ("index", a), ("bary", a), ("corner_order", a), ("corner_offsets", a), ("point_order", a), ("point_offsets", a),
        ("grad_triangles", a), ("grad_images", None), ("usable", None), ("dpoints", a), ("dvertices", a),
        ("stream", None))])
    for name in ("points", "vertices", "triangles", "index", "bary", "corner_order", "corner_offsets", "point_order",
                 "point_offsets"):
        assert bwd(**{name: None}) == EINVAL, name
    assert bwd(grad_triangles=None) == EINVAL              # no upstream
    assert bwd(grad_images=a) == EINVAL                    # two of them
    assert bwd(grad_triangles=None, grad_images=a) == EINVAL   # the mean's upstream without the count
    assert bwd(corner_order=None, corner_offsets=None) == EINVAL and bwd(point_order=None, point_offsets=None) == EINVAL
    for name, value in (("B", 0), ("N", 0), ("V", 0), ("T", 0), ("T", (1 << 28) + 1)):
        assert bwd(**{name: value}) == EINVAL, (name, value)


@pytest.mark.parametrize("c", mp.CASES, ids=mp.name)
def test_torch_path_matches_the_restatement(c):
    p, v, tri, lengths = mp.case(c)
    B, T = p.shape[0], tri.shape[0]
    pl, vl = p.clone().requires_grad_(True), v.clone().requires_grad_(True)
    sqdist, index, bary = points.triangle_nearest_points(pl, vl, tri, lengths)
    assert sqdist.shape == index.shape == (B, T) and bary.shape == (B, T, 3)
    assert sqdist.dtype == bary.dtype == torch.float32 and index.dtype == torch.int32
    assert sqdist.grad_fn is not None and not index.requires_grad and not bary.requires_grad
    errors = mp.forward_errors(p, v, tri, sqdist, index, bary, lengths, mp.HOST_BOUND_UNITS)
    mp.check_forward(errors, mp.HOST_BOUND_UNITS, "torch path %s" % mp.name(c), in_unit_cube=c[1] != "translated")
    g = torch.Generator().manual_seed(3)
    upstream = torch.randn(sqdist.shape, generator=g)
    sqdist.backward(upstream)
    wdp, wdv = mp.gradients(p, v, tri, index, bary, upstream)
    _grad_close(pl.grad, wdp, "%s dpoints" % mp.name(c))
    _grad_close(vl.grad, wdv, "%s dvertices" % mp.name(c))
    # the mean
    pl, vl = p.clone().requires_grad_(True), v.clone().requires_grad_(True)
    mean = points.mesh_point_distance(pl, vl, tri, lengths)
    assert mean.shape == (B,) and mean.dtype == torch.float32
    want, want_index, _ = mp.cached_nearest(c)
    want_mean = mp.mean_of(want, v, tri)
    atol = mp.mean_atol(p, v, tri, want_index, mp.HOST_BOUND_UNITS)
    assert bool(((mean.detach().double() - want_mean).abs() <= 1e-5 * want_mean + atol).all())
    weights = torch.randn(B, generator=g)
    mean.backward(weights)
    wdp, wdv = mp.mean_gradients(p, v, tri, index, bary, weights)
    _grad_close(pl.grad, wdp, "%s mean dpoints" % mp.name(c))
    _grad_close(vl.grad, wdv, "%s mean dvertices" % mp.name(c))


def test_thin_triangles_stay_between_the_minimum_and_the_nearest_edge():
    p, v, tri = ref.sliver_mesh()
    sqdist, index, bary = points.triangle_nearest_points(p, v, tri)
    mp.check_sliver(p, v, tri, sqdist, index, bary, mp.HOST_BOUND_UNITS, "torch path, thin triangles")


def test_the_face_distance_is_the_sum_of_its_halves():
    for c in (("ref", 3), ("own", 6)):
        p, v, tri, lengths = mp.case(c)
        pl, vl = p.clone().requires_grad_(True), v.clone().requires_grad_(True)
        both = points.point_mesh_face_distance(pl, vl, tri, lengths)
        halves = points.point_mesh_distance(p, v, tri, lengths) + points.mesh_point_distance(p, v, tri, lengths)
        assert both.shape == (p.shape[0],) and torch.equal(both.detach(), halves)
        both.sum().backward()
        assert bool(torch.isfinite(pl.grad).all()) and bool((vl.grad != 0).any())
    p, v, tri, _ = mp.case(("ref", 3))
    assert points.point_mesh_face_distance(p[0], v[0], tri).dim() == 0


def test_exact_ties_go_to_the_lowest_point():
    p, v, tri, _ = mp.case(("ref", 3))
    base = points.triangle_nearest_points(p, v, tri)
    again = points.triangle_nearest_points(torch.cat([p, p, p], dim=1), v, tri)
    for a, b in zip(base, again):
        assert torch.equal(a, b)


def test_lengths_and_poisoned_padding():
    p, v, tri, lengths = mp.case(("own", 6))            # lengths 700, 0, 333
    runs = []
    for poison in (None, float("nan"), float("inf"), 3.0e38):
        cloud = p.clone()
        if poison is not None:
            for b in range(p.shape[0]):
                cloud[b, int(lengths[b]):] = poison
        pl, vl = cloud.requires_grad_(True), v.clone().requires_grad_(True)
        out = points.triangle_nearest_points(pl, vl, tri, lengths)
        mean = points.mesh_point_distance(pl, vl, tri, lengths)
        (out[0].sum() + mean.sum()).backward()
        runs.append(tuple(t.detach() for t in out) + (mean.detach(), pl.grad, vl.grad))
    for other in runs[1:]:                     # the padding influences nothing, bit for bit
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    sqdist, index, bary, mean, dp, dv = runs[0]
    assert bool((index[0] >= 0).all()) and bool((index[2] >= 0).all()) and bool((index[2] < 333).all())
    # lengths = 0: no result, no gradient, a mean of 0
    assert bool((index[1] == -1).all()) and bool((sqdist[1] == 0).all()) and bool((bary[1] == 0).all())
    assert float(mean[1]) == 0.0 and bool((dp[1] == 0).all()) and bool((dv[1] == 0).all())
    assert bool((dp[2, 333:] == 0).all()) and bool(torch.isfinite(dv).all())
    # lengths beyond the cloud are clamped; a 0-dim length for a cloud without the batch axis
    over = points.triangle_nearest_points(p, v, tri, torch.tensor([9999, 700, 2 ** 40]))
    for a, b in zip(over, points.triangle_nearest_points(p, v, tri)):
        assert torch.equal(a, b)
    one = points.triangle_nearest_points(p[2], v[2], tri, lengths=torch.tensor(333))
    assert one[0].shape == (90,) and one[1].shape == (90,) and one[2].shape == (90, 3)
    for a, b in zip(one, (sqdist, index, bary)):
        assert torch.equal(a, b[2])


def test_unusable_triangles_and_non_finite_coordinates():
    p, v, tri, _ = mp.case(("ref", 4))
    B, N, V, T = ref.SHAPES[4]
    mixed = tri.clone()
    mixed[::2, 0] = -1
    mixed[1::4, 2] = V
    usable = ((mixed >= 0) & (mixed < V)).all(dim=1)
    sqdist, index, bary = points.triangle_nearest_points(p, v, mixed)
    mp.check_forward(mp.forward_errors(p, v, mixed, sqdist, index, bary, None, mp.HOST_BOUND_UNITS),
                     mp.HOST_BOUND_UNITS, "unusable triangles")
    assert bool((index[:, ~usable] == -1).all()) and bool((index[:, usable] >= 0).all())
    mean = points.mesh_point_distance(p, v, mixed)
    assert float((mean.double() - sqdist.double().sum(1) / int(usable.sum())).abs().max()) <= 1e-6 * float(mean.max())
    # all triangles unusable
    none = torch.full_like(tri, V)
    none[::3] = -1
    pl, vl = p.clone().requires_grad_(True), v.clone().requires_grad_(True)
    sqdist, index, bary = points.triangle_nearest_points(pl, vl, none)
    mean = points.mesh_point_distance(pl, vl, none)
    assert bool((index == -1).all()) and bool((sqdist == 0).all()) and bool((bary == 0).all()) and bool((mean == 0).all())
    (sqdist.sum() + mean.sum()).backward()
    assert bool((pl.grad == 0).all()) and bool((vl.grad == 0).all())
    # NaN and inf in some points and vertices: such a point is never chosen; a triangle that names such a vertex may
    # still have a finite edge, every other usable triangle has a result
    bad_p, bad_v = p.clone(), v.clone()
    bad_p[0, 5, 1] = float("nan")
    bad_p[1, 9, 0] = float("inf")
    bad_v[0, 7, 2] = float("nan")
    bad_v[1, 11, 0] = float("-inf")
    sqdist, index, bary = points.triangle_nearest_points(bad_p, bad_v, mixed)
    index = index.long()
    assert bool((index >= -1).all()) and bool((index < N).all())
    assert not bool((index[0] == 5).any()) and not bool((index[1] == 9).any())
    for b, vertex in ((0, 7), (1, 11)):
        names = (mixed == vertex).any(dim=1)
        assert bool((index[b, usable & ~names] >= 0).all()) and bool((index[b, ~usable] == -1).all())
    assert not bool(torch.isnan(bary).any())   # (sqdist is re-evaluated from the vertices here: 0 x NaN for such an edge)
    # a cloud of nothing but NaN: no result anywhere
    assert bool((points.triangle_nearest_points(torch.full_like(p, float("nan")), v, tri)[1] == -1).all())


def test_float64_input_forms_and_chunking(monkeypatch):
    p, v, tri, _ = mp.case(("ref", 4))
    want, want_index, _ = mp.cached_nearest(("ref", 4))
    sqdist, index, bary = points.triangle_nearest_points(p.double(), v.double(), tri)
    assert sqdist.dtype == bary.dtype == torch.float64 and index.dtype == torch.int32
    assert float((index.long() == want_index).double().mean()) > 0.99
    assert float((sqdist - want).abs().max()) <= 1e-12
    assert points.mesh_point_distance(p.double(), v.double(), tri).dtype == torch.float64
    # a chunk of a few triangles at a time gives the same answer
    whole = points.triangle_nearest_points(p, v, tri)
    monkeypatch.setattr(points, "_CHUNK_BYTES", 7 * 2 * 257 * 12 * 4)
    for a, b in zip(whole, points.triangle_nearest_points(p, v, tri)):
        assert torch.equal(a, b)
    monkeypatch.undo()
    # without the batch axis; int32 and int16 triangles; a non-contiguous view
    one = points.triangle_nearest_points(p[1], v[1], tri.to(torch.int16))
    assert one[0].shape == (1031,) and one[2].shape == (1031, 3)
    for a, b in zip(one, whole):
        assert torch.equal(a, b[1])
    assert points.mesh_point_distance(p[1], v[1], tri.to(torch.int32)).dim() == 0
    wide = torch.zeros(2, 257, 6)
    wide[..., 1::2] = p
    for a, b in zip(points.triangle_nearest_points(wide[..., 1::2], v, tri), whole):
        assert torch.equal(a, b)
    # no gradient wanted: no graph
    assert whole[0].grad_fn is None and points.mesh_point_distance(p, v, tri).grad_fn is None
    vl = v.clone().requires_grad_(True)
    points.mesh_point_distance(p, vl, tri).sum().backward()
    assert p.grad is None and vl.grad is not None


@pytest.mark.parametrize("function", ["triangle_nearest_points", "mesh_point_distance", "point_mesh_face_distance"])
def test_argument_checks(function):
    """Every error nearest_triangles raises (tests/test_point_mesh_host.py), for each of the new functions."""
    f = getattr(points, function)
    p, v, tri, _ = mp.case(("ref", 3))
    with pytest.raises(TypeError):
        f(p.numpy(), v, tri)
    with pytest.raises(TypeError):
        f(p.long(), v, tri)
    with pytest.raises(TypeError):
        f(p, v.long(), tri)
    with pytest.raises(TypeError):
        f(p, v, tri.tolist())
    with pytest.raises(RuntimeError):
        f(p, v, tri.float())
    with pytest.raises(RuntimeError):
        f(p, v.double(), tri)
    with pytest.raises(ValueError):
        f(p[..., :2], v, tri)
    with pytest.raises(ValueError):
        f(p[0], v, tri)                     # one with, one without the batch axis
    with pytest.raises(ValueError):
        f(p[:2], v, tri)
    with pytest.raises(ValueError):
        f(p, v, tri[:, :2])
    with pytest.raises(ValueError):
        f(p, v, tri[:0])
    with pytest.raises(ValueError):
        f(p, v, tri, lengths=torch.tensor([1, 2]))
    with pytest.raises(RuntimeError):
        f(p, v, tri, lengths=torch.tensor([1.0, 2.0, 3.0]))
    with pytest.raises(TypeError):
        f(p, v, tri, lengths=[1, 2, 3])


def test_the_library_takes_device_tensors_only():
    p, v, tri, _ = mp.case(("ref", 3))
    with pytest.raises(RuntimeError):
        _native.nearest_point_of_triangle_forward(p, v, tri.to(torch.int32))
