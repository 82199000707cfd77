"""mesh_renderer.points on the MI355X (csrc/nearest.hip) against the float64 restatement (tests/points_reference.py).

Budgets: sqdist within 1e-6 relative of float64 (the difference form costs one rounding each in the subtraction, the
product and the two sums, below 4 * 2^-24); Chamfer values within 1e-5 relative (a reordered float32 sum); the
float64 distance to the neighbour the kernel names within 1e-6 relative of the true minimum; the index equal to the
float64 argmin wherever the runner-up is further than 4e-6 relative (tests/test_points_host.py counts such points on
the CPU: none on any seeded shape); gradients within 1e-4 of the largest magnitude of the expected gradient tensor,
the restatement being evaluated with the kernel's own indices.

The shapes are ref.SHAPES: the issue's seven and three of ours, one point above queries_per_lane x workgroup size
(257 and 1025) and above the target tile (257) of nearest_plan.  (1, 40, 5000) splits under the shipped heuristic."""
import pytest
import torch

import points_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
points = mesh_renderer.points
reg = mesh_renderer.regularizers
CASES = list(range(len(ref.SHAPES))) + ["translated"]


def _clouds(k):
    return ref.translated_clouds() if k == "translated" else ref.clouds(k)


def _close(got, want, rel, what):
    err = (got.double().cpu() - want).abs()
    print("%s: max rel err %.3g" % (what, float((err / want.abs().clamp(min=1e-300)).max())))
    assert bool((err <= rel * want.abs()).all()), what


def _grad_close(got, want, what):
    scale = float(want.abs().max())
    err = float((got.double().cpu() - want).abs().max())
    print("%s: gradient max err %.3g of scale %.3g" % (what, err, scale))
    assert err <= 1e-4 * scale, "%s: gradient error %.3g > 1e-4 * %.3g" % (what, err, scale)


def test_the_shapes_cover_every_launch_path():
    plans = {}
    for B, N, M in ref.SHAPES:
        for shape in ((B, N, M), (B, M, N)):   # Chamfer runs both directions
            plans[shape] = _native.nearest_plan(*shape)
    assert plans[(1, 40, 5000)]["splits"] > 1
    for lanes in (1, 4):   # both query widths, each with and without a split
        assert any(p["queries_per_lane"] == lanes and p["splits"] == 1 for p in plans.values())
        assert any(p["queries_per_lane"] == lanes and p["splits"] > 1 for p in plans.values())
    for p in plans.values():
        assert p["target_tile"] == 256 and p["workgroup_size"] == 256
    one = _native.nearest_plan(1, 257, 257)
    wide = _native.nearest_plan(2, 1025, 257)
    assert one["queries_per_lane"] * one["workgroup_size"] + 1 == 257 and one["target_tile"] + 1 == 257
    assert wide["queries_per_lane"] * wide["workgroup_size"] + 1 == 1025


@pytest.mark.parametrize("k", CASES)
def test_nearest_points_matches_the_restatement(k):
    x, y = _clouds(k)
    want, want_idx, gap = ref.nearest(x, y) if k == "translated" else ref.cached_nearest(k)
    xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    got, idx = points.nearest_points(xg, yg)
    assert got.shape == idx.shape == x.shape[:2] and got.dtype == torch.float32 and idx.dtype == torch.int32
    assert got.is_cuda and not idx.requires_grad and got.grad_fn is not None
    idx_host = idx.cpu()
    assert bool((idx_host >= 0).all()) and bool((idx_host < y.shape[1]).all())
    _close(got.detach(), want, 1e-6, "%s sqdist" % (k,))
    _close(ref.distance_to(x, y, idx_host), want, 1e-6, "%s distance to the named neighbour" % (k,))
    clear = gap > ref.RUNNER_UP_MARGIN
    assert int((~clear).sum()) <= 0.01 * clear.numel()
    assert torch.equal(idx_host.long()[clear], want_idx[clear])
    g = torch.Generator().manual_seed(3)
    upstream = torch.randn(got.shape, generator=g)
    got.backward(upstream.to(DEV))
    wdx, wdy = ref.nearest_gradients(x, y, idx_host, upstream)
    _grad_close(xg.grad, wdx, "%s dx" % (k,))
    _grad_close(yg.grad, wdy, "%s dy" % (k,))


@pytest.mark.parametrize("k", CASES)
def test_chamfer_distance_matches_the_restatement(k):
    x, y = _clouds(k)
    want = ref.chamfer(x, y, x_weight=0.75, y_weight=1.5)
    xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    total = points.chamfer_distance(xg, yg, x_weight=0.75, y_weight=1.5)
    assert total.shape == (x.shape[0],) and total.dtype == torch.float32
    _close(total.detach(), want, 1e-5, "%s chamfer" % (k,))
    g = torch.Generator().manual_seed(4)
    upstream = torch.randn(x.shape[0], generator=g)
    total.backward(upstream.to(DEV))
    idx_xy = points.nearest_points(x.to(DEV), y.to(DEV))[1].cpu()   # the indices the same kernel gave the loss
    idx_yx = points.nearest_points(y.to(DEV), x.to(DEV))[1].cpu()
    wdx, wdy = ref.chamfer_gradients(x, y, idx_xy, idx_yx, upstream, x_weight=0.75, y_weight=1.5)
    _grad_close(xg.grad, wdx, "%s chamfer dx" % (k,))
    _grad_close(yg.grad, wdy, "%s chamfer dy" % (k,))
    # one direction alone
    for weights in ((0.0, 1.0), (2.0, 0.0)):
        one = points.chamfer_distance(x.to(DEV), y.to(DEV), x_weight=weights[0], y_weight=weights[1])
        _close(one, ref.chamfer(x, y, x_weight=weights[0], y_weight=weights[1]), 1e-5, "%s chamfer %s" % (k, weights))


@pytest.mark.parametrize("wide", [False, True])
def test_exact_ties_go_to_the_lowest_index(wide):
    x, y = ref.lattice_clouds(wide)
    plan = _native.nearest_plan(1, x.shape[1], y.shape[1])
    assert (plan["splits"] > 1) == wide
    want, want_idx, _ = ref.nearest(x, y)
    assert bool((want == 0.75).all())
    got, idx = points.nearest_points(x.to(DEV), y.to(DEV))
    assert torch.equal(got.double().cpu(), want)      # exact in float32 under any contraction
    assert torch.equal(idx.cpu().long(), want_idx)
    # the reverse direction: every lattice point has ties among the cells around it
    want, want_idx, _ = ref.nearest(y, x)
    got, idx = points.nearest_points(y.to(DEV), x.to(DEV))
    assert torch.equal(got.double().cpu(), want) and torch.equal(idx.cpu().long(), want_idx)


def test_lengths_and_poisoned_padding():
    x, y = ref.clouds(4)                       # (2, 257, 1031): x -> y splits, y -> x does not
    x, y = torch.cat([x, x[:1], x[1:]]), torch.cat([y, y[:1], y[1:]])   # four images
    xl, yl = torch.tensor([257, 100, 0, 257]), torch.tensor([1031, 300, 1031, 0])
    poisoned_x, poisoned_y = x.clone(), y.clone()
    for b in range(4):
        poisoned_x[b, int(xl[b]):] = 1e30
        poisoned_y[b, int(yl[b]):] = 1e30
    want, want_idx, gap = ref.nearest(x, y, xl, yl)
    assert int((gap <= ref.RUNNER_UP_MARGIN).sum()) == 0
    runs = []
    for cx, cy in ((x, y), (poisoned_x, poisoned_y)):
        xg, yg = cx.to(DEV).requires_grad_(True), cy.to(DEV).requires_grad_(True)
        got, idx = points.nearest_points(xg, yg, xl.to(DEV), yl.to(DEV))
        g = torch.Generator().manual_seed(5)
        upstream = torch.randn(got.shape, generator=g)
        got.backward(upstream.to(DEV))
        total = points.chamfer_distance(xg, yg, xl.to(DEV), yl.to(DEV))
        cgx, cgy = torch.autograd.grad(total.sum(), (xg, yg))
        runs.append((got.detach(), idx, xg.grad, yg.grad, total.detach(), cgx, cgy))
    got, idx, dx, dy, total, cgx, cgy = runs[0]
    for a, b in zip(runs[0], runs[1]):        # the padding influences nothing, bit for bit
        assert torch.equal(a, b)
    assert torch.equal(idx.cpu().long(), want_idx)
    _close(got, want, 1e-6, "padded sqdist")
    assert bool((idx[2:] == -1).all()) and bool((got[2:] == 0).all())
    assert bool((idx[1, 100:] == -1).all()) and bool((got[1, 100:] == 0).all()) and bool((idx[1, :100] < 300).all())
    wdx, wdy = ref.nearest_gradients(x, y, idx.cpu(), upstream)
    _grad_close(dx, wdx, "padded dx")
    _grad_close(dy, wdy, "padded dy")
    assert bool((dx[1, 100:] == 0).all()) and bool((dx[2:] == 0).all())
    assert bool((dy[1, 300:] == 0).all()) and bool((dy[2:] == 0).all())
    want_total = ref.chamfer(x, y, xl, yl)
    _close(total, want_total, 1e-5, "padded chamfer")
    assert float(total[2]) == 0.0 and float(total[3]) == 0.0
    idx_yx = points.nearest_points(y.to(DEV), x.to(DEV), yl.to(DEV), xl.to(DEV))[1].cpu()
    wcx, wcy = ref.chamfer_gradients(x, y, idx.cpu(), idx_yx, torch.ones(4), xl, yl)
    _grad_close(cgx, wcx, "padded chamfer dx")
    _grad_close(cgy, wcy, "padded chamfer dy")
    assert bool((cgx[1, 100:] == 0).all()) and bool((cgx[2:] == 0).all()) and bool((cgy[1, 300:] == 0).all())
    # lengths beyond the clouds are clamped by the kernel, int64 lengths are taken
    over = points.nearest_points(x.to(DEV), y.to(DEV), torch.tensor([9999, 257, 300, 257], device=DEV),
                                 torch.tensor([1031, 2 ** 40, 5000, 1031], device=DEV))
    plain = points.nearest_points(x.to(DEV), y.to(DEV))
    assert torch.equal(over[0], plain[0]) and torch.equal(over[1], plain[1])


@pytest.mark.parametrize("k", [3, 4])   # without and with a split
def test_non_finite_coordinates_keep_the_indices_in_range(k):
    x, y = ref.clouds(k)
    B, N, M = ref.SHAPES[k]
    clean, clean_idx = points.nearest_points(x.to(DEV), y.to(DEV))
    bad_x, bad_y = x.clone(), y.clone()
    bad_x[0, 5, 1] = float("nan")
    bad_y[0, 7, 2] = float("nan")
    xg, yg = bad_x.to(DEV).requires_grad_(True), bad_y.to(DEV).requires_grad_(True)
    got, idx = points.nearest_points(xg, yg)
    assert bool((idx >= 0).all()) and bool((idx < M).all())
    unaffected = clean_idx != 7
    unaffected[1:] = True
    unaffected[0, 5] = False
    assert torch.equal(got[unaffected], clean[unaffected]) and torch.equal(idx[unaffected], clean_idx[unaffected])
    assert bool((idx[0] != 7).all())      # a NaN distance never wins
    got.sum().backward()                   # reads nothing out of range; the values may be non-finite
    total = points.chamfer_distance(xg, yg)
    total.sum().backward()
    assert bool(torch.isfinite(total[1:]).all())
    both = points.nearest_points(yg.detach(), xg.detach())[1]
    assert bool((both >= 0).all()) and bool((both < N).all())


def test_input_forms():
    x, y = ref.clouds(3)
    want, want_idx, _ = ref.cached_nearest(3)
    # a non-contiguous view
    wide = torch.zeros(3, 65, 6, device=DEV)
    wide[..., 1::2] = x.to(DEV)
    leaf = wide.requires_grad_(True)
    view = leaf[..., 1::2]
    assert not view.is_contiguous()
    yd = y.to(DEV)
    got, idx = points.nearest_points(view, yd)
    _close(got.detach(), want, 1e-6, "non-contiguous x")
    assert torch.equal(idx.cpu().long(), want_idx)
    upstream = torch.ones_like(got)
    got.backward(upstream)
    wdx, _ = ref.nearest_gradients(x, y, idx.cpu(), upstream.cpu())
    _grad_close(leaf.grad[..., 1::2], wdx, "non-contiguous dx")
    assert bool((leaf.grad[..., 0::2] == 0).all())
    assert yd.grad is None                 # requires_grad on one cloud only
    # the other cloud alone, through Chamfer
    xd = x.to(DEV)
    yg = y.to(DEV).requires_grad_(True)
    points.chamfer_distance(xd, yg).sum().backward()
    assert xd.grad is None and yg.grad is not None and bool(torch.isfinite(yg.grad).all())
    _, wdy = ref.chamfer_gradients(x, y, idx.cpu(), points.nearest_points(yd, xd)[1].cpu(), torch.ones(3))
    _grad_close(yg.grad, wdy, "chamfer dy alone")
    # no gradient wanted: no backward node
    assert points.chamfer_distance(xd, yd).grad_fn is None and points.nearest_points(xd, yd)[0].grad_fn is None
    # [N,3] clouds, int64 lengths
    d, i = points.nearest_points(xd[1], yd[1], y_lengths=torch.tensor([40], device=DEV, dtype=torch.int64))
    w, wi, _ = ref.nearest(x[1:2], y[1:2], None, torch.tensor([40]))
    assert d.shape == (65,) and torch.equal(i.cpu().long(), wi[0])
    _close(d, w[0], 1e-6, "[N,3] clouds")
    c = points.chamfer_distance(xd[1], yd[1])
    assert c.dim() == 0
    _close(c, ref.chamfer(x[1:2], y[1:2])[0], 1e-5, "[N,3] chamfer")
    with pytest.raises(RuntimeError):
        points.nearest_points(xd, y)       # clouds on two devices
    with pytest.raises(RuntimeError):
        points.nearest_points(xd, yd, x_lengths=torch.tensor([1, 2, 3]))   # lengths on the host


def test_bitwise_reproducible_in_either_mode():
    x, y = ref.clouds(4)
    g = torch.Generator().manual_seed(6)
    upstream = torch.randn(2, 257, generator=g).to(DEV)

    def run():
        xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
        got, idx = points.nearest_points(xg, yg)
        got.backward(upstream)
        total = points.chamfer_distance(xg, yg)
        cgx, cgy = torch.autograd.grad(total.sum(), (xg, yg))
        return got.detach(), idx, xg.grad, yg.grad, total.detach(), cgx, cgy

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


def test_captured_step_with_chamfer_and_the_regulariser():
    vertices, triangles, _ = shapes.sphere(1.0, 6)
    B, V = 2, vertices.shape[0]
    tri = triangles.to(DEV)
    g = torch.Generator().manual_seed(9)
    v = (vertices[None] + 0.03 * torch.randn(B, V, 3, generator=g)).to(DEV).requires_grad_(True)
    scan = (torch.randn(B, 700, 3, generator=g) * torch.tensor([1.4, 0.8, 1.0])).to(DEV)
    lengths = torch.tensor([700, 450], device=DEV)
    reg.mesh_topology(tri, V)              # reads counts back: built before the capture

    def loss_of(m):
        return (points.chamfer_distance(m, scan, y_lengths=lengths) + reg.mesh_regularizer(m, tri, 0.3, 0.2, 0.1)).sum()

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
    # the Chamfer part of the replayed step is the restatement's
    only = v.detach().clone().requires_grad_(True)
    total = points.chamfer_distance(only, scan, y_lengths=lengths)
    total.sum().backward()
    host_v, host_scan, host_len = v.detach().cpu(), scan.cpu(), lengths.cpu()
    _close(total.detach(), ref.chamfer(host_v, host_scan, None, host_len), 1e-5, "captured chamfer")
    idx_xy = points.nearest_points(v.detach(), scan, None, lengths)[1].cpu()
    idx_yx = points.nearest_points(scan, v.detach(), lengths, None)[1].cpu()
    wdx, _ = ref.chamfer_gradients(host_v, host_scan, idx_xy, idx_yx, torch.ones(B), None, host_len)
    _grad_close(only.grad, wdx, "captured chamfer dx")
