"""mesh_renderer.points.nearest_triangles / point_mesh_distance on the MI355X (the k_nt_* kernels of csrc/nearest.hip)
against the float64 restatement (tests/point_mesh_reference.py).

Forward bound: ref.HIP_BOUND_UNITS = 4 x the worst error of the package's float32 torch path on the CPU (1.74, so
6.96) in units of 2^-24 * scale_i, scale_i = max_k |p_i - v_k|^2 over the corners of the named face, for
|sqdist - min|, for the float64 distance to the named face above the minimum, and (twice the bound) for the float64
distance at the returned barycentrics -- no query exempt.  Gradients: within 1e-4 of the largest magnitude of the
expected gradient tensor (_grad_close of tests/test_points_gpu.py), the restatement evaluated with the returned
(face, bary).  The shapes are ref.SHAPES: the issue's six and three of ours, one query above queries_per_lane x
workgroup size (257, 513) and one triangle above the tile (129) of nearest_triangle_plan."""
import pytest
import torch

import point_mesh_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
points = mesh_renderer.points
reg = mesh_renderer.regularizers
CASES = list(range(len(ref.SHAPES))) + ["translated"]


def _grad_close(got, want, what):
    scale = float(want.abs().max())
    err = float((got.double().cpu() - want).abs().max())
    print("%s: gradient max err %.3g of scale %.3g" % (what, err, scale))
    assert err <= 1e-4 * scale, "%s: gradient error %.3g > 1e-4 * %.3g" % (what, err, scale)


def _check(p, v, tri, out, what, lengths=None, in_unit_cube=True):
    sqdist, face, bary = out
    assert sqdist.shape == face.shape == p.shape[:2] and bary.shape == p.shape
    assert sqdist.dtype == bary.dtype == torch.float32 and face.dtype == torch.int32
    assert sqdist.is_cuda and face.is_cuda and bary.is_cuda and not face.requires_grad and not bary.requires_grad
    errors = ref.forward_errors(p, v, tri, sqdist, face, bary, lengths)
    ref.check_forward(errors, ref.HIP_BOUND_UNITS, what, in_unit_cube)


@pytest.mark.parametrize("k", CASES)
def test_nearest_triangles_matches_the_restatement(k):
    p, v, tri = ref.mesh(k)
    pg, vg = p.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    sqdist, face, bary = points.nearest_triangles(pg, vg, tri.to(DEV))
    assert sqdist.grad_fn is not None
    _check(p, v, tri, (sqdist, face, bary), "%s" % (k,), in_unit_cube=k != "translated")
    assert bool((face >= 0).all())
    g = torch.Generator().manual_seed(3)
    upstream = torch.randn(sqdist.shape, generator=g)
    sqdist.backward(upstream.to(DEV))
    wdp, wdv = ref.gradients(p, v, tri, face.cpu(), bary.cpu(), upstream)
    _grad_close(pg.grad, wdp, "%s dpoints" % (k,))
    _grad_close(vg.grad, wdv, "%s dvertices" % (k,))
    # each gradient alone
    alone = p.to(DEV).requires_grad_(True)
    points.nearest_triangles(alone, v.to(DEV), tri.to(DEV))[0].backward(upstream.to(DEV))
    assert torch.equal(alone.grad, pg.grad)
    alone = v.to(DEV).requires_grad_(True)
    points.nearest_triangles(p.to(DEV), alone, tri.to(DEV))[0].backward(upstream.to(DEV))
    assert torch.equal(alone.grad, vg.grad)


@pytest.mark.parametrize("k", CASES)
def test_point_mesh_distance_matches_the_restatement(k):
    p, v, tri = ref.mesh(k)
    want, want_face = ref.cached_nearest(k) if k != "translated" else ref.nearest(p, v, tri)
    pg, vg = p.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    mean = points.point_mesh_distance(pg, vg, tri.to(DEV))
    assert mean.shape == (p.shape[0],) and mean.dtype == torch.float32 and mean.is_cuda
    want_mean = ref.mean_of(want)
    atol = ref.mean_atol(p, v, tri, want_face, ref.HIP_BOUND_UNITS)
    err = (mean.detach().double().cpu() - want_mean).abs()
    print("%s mean: err %s of %s" % (k, err.tolist(), want_mean.tolist()))
    assert bool((err <= 1e-5 * want_mean + atol).all())
    g = torch.Generator().manual_seed(4)
    upstream = torch.randn(p.shape[0], generator=g)
    mean.backward(upstream.to(DEV))
    _, face, bary = points.nearest_triangles(p.to(DEV), v.to(DEV), tri.to(DEV))   # what the same kernels gave the loss
    wdp, wdv = ref.mean_gradients(p, v, tri, face.cpu(), bary.cpu(), upstream)
    _grad_close(pg.grad, wdp, "%s mean dpoints" % (k,))
    _grad_close(vg.grad, wdv, "%s mean dvertices" % (k,))
    alone = v.to(DEV).requires_grad_(True)
    points.point_mesh_distance(p.to(DEV), alone, tri.to(DEV)).backward(upstream.to(DEV))
    assert torch.equal(alone.grad, vg.grad) and pg.grad is not None
    alone = p.to(DEV).requires_grad_(True)
    points.point_mesh_distance(alone, v.to(DEV), tri.to(DEV)).backward(upstream.to(DEV))
    assert torch.equal(alone.grad, pg.grad)


@pytest.mark.parametrize("split", [False, True])
def test_exact_ties_go_to_the_lowest_face(split):
    """The same triangles listed four times over are identical arithmetic: the lowest copy wins inside one tile
    (4 x 30 triangles) and across the splits (4 x 150 triangles, 40 queries: every copy in another chunk)."""
    count = 150 if split else 30
    p, v, tri = ref.mesh(5 if split else 3)
    tri = tri[:count]
    plan = _native.nearest_triangle_plan(p.shape[0], p.shape[1], 4 * count)
    assert (plan["splits"] > 1) == split
    if split:
        tiles = -(-4 * count // plan["triangle_tile"])
        chunk = -(-tiles // plan["splits"]) * plan["triangle_tile"]
        assert chunk <= count                   # the copies of a face lie in different chunks
    base = points.nearest_triangles(p.to(DEV), v.to(DEV), tri.to(DEV))
    again = points.nearest_triangles(p.to(DEV), v.to(DEV), torch.cat([tri] * 4).to(DEV))
    _check(p, v, tri, base, "ties, one copy")
    assert bool((again[1] < count).all())
    for a, b in zip(base, again):
        assert torch.equal(a, b)


def test_degenerate_triangles_alone():
    p, v, tri = ref.degenerate_mesh()
    pg, vg = p.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    sqdist, face, bary = points.nearest_triangles(pg, vg, tri.to(DEV))
    assert bool(torch.isfinite(sqdist).all()) and bool((face >= 0).all())
    _check(p, v, tri, (sqdist, face, bary), "degenerate mesh")
    g = torch.Generator().manual_seed(8)
    upstream = torch.randn(sqdist.shape, generator=g)
    sqdist.backward(upstream.to(DEV))
    assert bool(torch.isfinite(pg.grad).all()) and bool(torch.isfinite(vg.grad).all())
    wdp, wdv = ref.gradients(p, v, tri, face.cpu(), bary.cpu(), upstream)
    _grad_close(pg.grad, wdp, "degenerate dpoints")
    _grad_close(vg.grad, wdv, "degenerate dvertices")


def test_thin_triangles_stay_between_the_minimum_and_the_nearest_edge():
    p, v, tri = ref.sliver_mesh()
    sqdist, face, bary = points.nearest_triangles(p.to(DEV), v.to(DEV), tri.to(DEV))
    ref.check_sliver(p, v, tri, sqdist, face, bary, ref.HIP_BOUND_UNITS, "thin triangles")


def test_lengths_and_poisoned_padding():
    p, v, tri = ref.mesh(4)                    # (2, 257, 200, 1031): splits
    p, v = torch.cat([p, p[:1], p[1:]]), torch.cat([v, v[:1], v[1:]])   # four images
    lengths = torch.tensor([257, 100, 0, 1])
    poisoned = p.clone()
    for b in range(4):
        poisoned[b, int(lengths[b]):] = float("nan")
    g = torch.Generator().manual_seed(5)
    upstream = torch.randn(4, 257, generator=g)
    runs = []
    for cloud in (p, poisoned):
        pg, vg = cloud.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
        out = points.nearest_triangles(pg, vg, tri.to(DEV), lengths.to(DEV))
        out[0].backward(upstream.to(DEV))
        mean = points.point_mesh_distance(pg, vg, tri.to(DEV), lengths.to(DEV))
        mp, mv = torch.autograd.grad(mean.sum(), (pg, vg))
        runs.append(tuple(t.detach() for t in out) + (pg.grad, vg.grad, mean.detach(), mp, mv))
    for a, b in zip(*runs):                    # the padding influences nothing, bit for bit
        assert torch.equal(a, b)
    sqdist, face, bary, dp, dv, mean, mp, mv = runs[0]
    _check(p, v, tri, (sqdist, face, bary), "padded", lengths)
    for b in range(4):
        n = int(lengths[b])
        assert bool((face[b, :n] >= 0).all()) and bool((face[b, n:] == -1).all())
        assert bool((sqdist[b, n:] == 0).all()) and bool((bary[b, n:] == 0).all())
        assert bool((dp[b, n:] == 0).all()) and bool((mp[b, n:] == 0).all())
    assert bool((dv[2] == 0).all()) and bool((mv[2] == 0).all()) and float(mean[2]) == 0.0
    wdp, wdv = ref.gradients(p, v, tri, face.cpu(), bary.cpu(), upstream)
    _grad_close(dp, wdp, "padded dpoints")
    _grad_close(dv, wdv, "padded dvertices")
    want, want_face = ref.nearest(p, v, tri, lengths)
    want_mean = ref.mean_of(want, lengths)
    atol = ref.mean_atol(p, v, tri, want_face, ref.HIP_BOUND_UNITS, lengths)
    assert bool(((mean.double().cpu() - want_mean).abs() <= 1e-5 * want_mean + atol).all())
    wmp, wmv = ref.mean_gradients(p, v, tri, face.cpu(), bary.cpu(), torch.ones(4), lengths)
    _grad_close(mp, wmp, "padded mean dpoints")
    _grad_close(mv, wmv, "padded mean dvertices")
    # lengths beyond the cloud are clamped by the kernel, int64 lengths are taken
    over = points.nearest_triangles(p.to(DEV), v.to(DEV), tri.to(DEV), torch.tensor([9999, 257, 2 ** 40, 300], device=DEV))
    plain = points.nearest_triangles(p.to(DEV), v.to(DEV), tri.to(DEV))
    for a, b in zip(over, plain):
        assert torch.equal(a, b)


@pytest.mark.parametrize("k", [3, 4])   # without and with a split
def test_unusable_triangles_are_never_chosen(k):
    p, v, tri = ref.mesh(k)
    V, T = ref.SHAPES[k][2], ref.SHAPES[k][3]
    assert (_native.nearest_triangle_plan(p.shape[0], p.shape[1], T)["splits"] > 1) == (k == 4)
    mixed = tri.clone()
    mixed[::2, 0] = -1
    mixed[1::4, 2] = V
    usable = ((mixed >= 0) & (mixed < V)).all(dim=1)
    out = points.nearest_triangles(p.to(DEV), v.to(DEV), mixed.to(DEV))
    _check(p, v, mixed, out, "unusable triangles %d" % k)
    face = out[1].cpu().long()
    assert bool((face >= 0).all()) and bool(usable[face].all())
    # nothing usable at all
    none = torch.full_like(tri, V)
    none[::3] = -1
    pg, vg = p.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    sqdist, face, bary = points.nearest_triangles(pg, vg, none.to(DEV))
    mean = points.point_mesh_distance(pg, vg, none.to(DEV))
    assert bool((face == -1).all()) and bool((sqdist == 0).all()) and bool((bary == 0).all()) and bool((mean == 0).all())
    (sqdist.sum() + mean.sum()).backward()
    assert bool((pg.grad == 0).all()) and bool((vg.grad == 0).all())


@pytest.mark.parametrize("k", [3, 4])   # without and with a split
def test_non_finite_coordinates_keep_the_faces_in_range(k):
    p, v, tri = ref.mesh(k)
    V, T = ref.SHAPES[k][2], ref.SHAPES[k][3]
    mixed = tri.clone()
    mixed[::5, 1] = V
    usable = ((mixed >= 0) & (mixed < V)).all(dim=1)
    clean = points.nearest_triangles(p.to(DEV), v.to(DEV), mixed.to(DEV))
    bad_p, bad_v = p.clone(), v.clone()
    bad_p[0, 5, 1] = float("nan")
    bad_p[1, 9, 0] = float("inf")
    bad_v[0, 7, 2] = float("nan")
    bad_v[1, 11, 0] = float("-inf")
    pg, vg = bad_p.to(DEV).requires_grad_(True), bad_v.to(DEV).requires_grad_(True)
    sqdist, face, bary = points.nearest_triangles(pg, vg, mixed.to(DEV))
    host = face.cpu().long()
    assert int(host[0, 5]) == -1 and int(host[1, 9]) == -1
    assert bool((host >= -1).all()) and bool((host < T).all()) and bool(usable[host[host >= 0]].all())
    names = lambda b, vertex: (mixed[clean[1][b].cpu().long()] == vertex).any(dim=1)
    for b, vertex, query in ((0, 7, 5), (1, 11, 9)):        # rows that never met the poisoned vertex are unchanged
        same = ~names(b, vertex) & ~(mixed[host[b].clamp(min=0)] == vertex).any(dim=1)
        same[query] = False
        assert bool(same.any())
        assert torch.equal(sqdist[b][same.to(DEV)], clean[0][b][same.to(DEV)])
        assert torch.equal(face[b][same.to(DEV)], clean[1][b][same.to(DEV)])
    sqdist.sum().backward()                    # reads nothing out of range; the values may be non-finite
    mean = points.point_mesh_distance(pg, vg, mixed.to(DEV))
    mean.sum().backward()
    torch.cuda.synchronize()


def test_input_forms():
    p, v, tri = ref.mesh(3)
    pd, vd, td = p.to(DEV), v.to(DEV), tri.to(DEV)
    whole = points.nearest_triangles(pd, vd, td)
    # a non-contiguous view, and its gradient
    wide = torch.zeros(3, 65, 6, device=DEV)
    wide[..., 1::2] = pd
    leaf = wide.requires_grad_(True)
    view = leaf[..., 1::2]
    assert not view.is_contiguous()
    out = points.nearest_triangles(view, vd, td.t().contiguous().t())
    for a, b in zip(out, whole):
        assert torch.equal(a.detach(), b)
    upstream = torch.ones_like(out[0])
    out[0].backward(upstream)
    wdp, _ = ref.gradients(p, v, tri, out[1].cpu(), out[2].cpu(), upstream.cpu())
    _grad_close(leaf.grad[..., 1::2], wdp, "non-contiguous dpoints")
    assert bool((leaf.grad[..., 0::2] == 0).all()) and vd.grad is None
    # every integer dtype of the triangles, on the host too
    for dtype in (torch.int64, torch.int32, torch.int16):
        for a, b in zip(points.nearest_triangles(pd, vd, tri.to(dtype)), whole):
            assert torch.equal(a, b)
    # no gradient wanted: no backward node
    assert whole[0].grad_fn is None and points.point_mesh_distance(pd, vd, td).grad_fn is None
    # without the batch axis, a 0-dim length
    one = points.nearest_triangles(pd[1], vd[1], td, lengths=torch.tensor(40, device=DEV))
    assert one[0].shape == (65,) and one[1].shape == (65,) and one[2].shape == (65, 3)
    for a, b in zip(one, whole):
        assert torch.equal(a[:40], b[1, :40])
    assert bool((one[1][40:] == -1).all())
    mean = points.point_mesh_distance(pd[1], vd[1], td)
    assert mean.dim() == 0 and abs(float(mean) - float(whole[0][1].double().mean())) <= 1e-5 * float(mean)
    # float64 on the device takes the torch path
    sqdist, face, bary = points.nearest_triangles(pd.double(), vd.double(), td)
    want, want_face = ref.cached_nearest(3)
    assert sqdist.dtype == torch.float64 and sqdist.is_cuda and face.dtype == torch.int32
    assert float((sqdist.cpu() - want).abs().max()) <= 1e-12
    with pytest.raises(RuntimeError):
        points.nearest_triangles(pd, v, td)    # points and vertices on two devices
    with pytest.raises(RuntimeError):
        points.nearest_triangles(pd, vd, td, lengths=torch.tensor([1, 2, 3]))   # lengths on the host
    with pytest.raises(RuntimeError):
        points.nearest_triangles(pd, vd.double(), td)
    with pytest.raises(ValueError):
        points.nearest_triangles(pd, vd[:2], td)
    with pytest.raises(TypeError):
        points.nearest_triangles(pd, vd, tri.tolist())


def test_bitwise_reproducible_in_either_mode():
    p, v, tri = ref.mesh(4)
    g = torch.Generator().manual_seed(6)
    upstream = torch.randn(2, 257, generator=g).to(DEV)
    td = tri.to(DEV)

    def run():
        pg, vg = p.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
        sqdist, face, bary = points.nearest_triangles(pg, vg, td)
        sqdist.backward(upstream)
        mean = points.point_mesh_distance(pg, vg, td)
        mp, mv = torch.autograd.grad(mean.sum(), (pg, vg))
        return sqdist.detach(), face, bary, pg.grad, vg.grad, mean.detach(), mp, mv

    before = _native.set_deterministic(False)
    try:
        runs = []
        for mode in (False, False, True, True):
            _native.set_deterministic(mode)
            runs.append(run())
    finally:
        _native.set_deterministic(before)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


def test_captured_step_with_the_point_mesh_distance_and_the_regulariser():
    vertices, triangles, _ = shapes.sphere(1.0, 6)
    B, V = 2, vertices.shape[0]
    tri = triangles.to(DEV)
    g = torch.Generator().manual_seed(9)
    v = (vertices[None] + 0.03 * torch.randn(B, V, 3, generator=g)).to(DEV).requires_grad_(True)
    scan = (torch.randn(B, 700, 3, generator=g) * torch.tensor([1.4, 0.8, 1.0])).to(DEV)
    lengths = torch.tensor([700, 450], device=DEV)
    reg.mesh_topology(tri, V)              # reads counts back: built before the capture

    def loss_of(m):
        return (points.point_mesh_distance(scan, m, tri, lengths) + reg.mesh_regularizer(m, tri, 0.3, 0.2, 0.1)).sum()

    def step():
        loss = loss_of(v)
        loss.backward()
        return loss

    captured = mesh_renderer.capture_step(step, [v])
    with torch.no_grad():
        v.add_(0.05 * torch.randn(B, V, 3, generator=g).to(DEV))
    loss = captured.replay().clone()
    grad = v.grad.clone()
    fresh = v.detach().clone().requires_grad_(True)
    eager = loss_of(fresh)
    eager.backward()
    assert torch.equal(loss, eager.detach()) and torch.equal(grad, fresh.grad)
    # the point-to-mesh part of the replayed step is the restatement's
    only = v.detach().clone().requires_grad_(True)
    mean = points.point_mesh_distance(scan, only, tri, lengths)
    mean.sum().backward()
    host_v, host_scan, host_tri, host_len = v.detach().cpu(), scan.cpu(), triangles, lengths.cpu()
    want, want_face = ref.nearest(host_scan, host_v, host_tri, host_len)
    want_mean = ref.mean_of(want, host_len)
    atol = ref.mean_atol(host_scan, host_v, host_tri, want_face, ref.HIP_BOUND_UNITS, host_len)
    assert bool(((mean.detach().double().cpu() - want_mean).abs() <= 1e-5 * want_mean + atol).all())
    _, face, bary = points.nearest_triangles(scan, v.detach(), tri, lengths)
    _, wdv = ref.mean_gradients(host_scan, host_v, host_tri, face.cpu(), bary.cpu(), torch.ones(B), host_len)
    _grad_close(only.grad, wdv, "captured point-to-mesh dvertices")
