"""mesh_renderer.points.knn_points / estimate_point_normals on the MI355X (csrc/nearest.hip, "K nearest neighbours")
against the float64 restatement (tests/knn_reference.py).

Budgets, taken from tests/test_points_gpu.py: sqdist within 1e-6 relative of float64 (the difference form costs one
rounding each in the subtraction, the product and the two sums, below 4 * 2^-24); the float64 distance to each named
neighbour within 1e-6 relative of the true k-th distance; idx equal to the float64 result in every slot whose gaps to
both adjacent neighbours exceed RUNNER_UP_MARGIN (4e-6 relative), such unclear slots being at most 0.1 % of the slots
of any (shape, K) (tests/test_knn_host.py counts them: 12 of 32 800 at worst); gradients within 1e-4 of the largest
magnitude of the expected tensor, the restatement being evaluated with the kernel's own indices.

The shapes are points_reference.SHAPES and the translated cloud; (1, 40, 5000) splits, and between them the plans
cover every list capacity with and without a split and every number of queries per lane."""
import pytest
import torch

import knn_reference as kref
import points_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
points = mesh_renderer.points
CASES = list(range(len(ref.SHAPES))) + ["translated"]
_device_clouds = {}


def _clouds(k):
    return ref.translated_clouds() if k == "translated" else ref.clouds(k)


def _on_device(k):
    if k not in _device_clouds:
        x, y = _clouds(k)
        _device_clouds[k] = (x.to(DEV), y.to(DEV))
    return _device_clouds[k]


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
    plans = {(shape, K): _native.knn_plan(*shape, K) for shape in ref.SHAPES for K in kref.KS}
    for K in kref.KS:
        assert plans[((1, 40, 5000), K)]["splits"] > 1
    for capacity in (4, 8, 16, 32):   # every list capacity, with and without a split
        assert any(p["list_capacity"] == capacity and p["splits"] == 1 for p in plans.values())
        assert any(p["list_capacity"] == capacity and p["splits"] > 1 for p in plans.values())
    for lanes in (1, 2, 4):           # every number of queries per lane, with and without a split
        assert any(p["queries_per_lane"] == lanes and p["splits"] == 1 for p in plans.values())
        assert any(p["queries_per_lane"] == lanes and p["splits"] > 1 for p in plans.values())
    assert {(p["list_capacity"], p["queries_per_lane"]) for p in plans.values()} == {(4, 1), (4, 4), (8, 1), (8, 2),
                                                                                      (16, 1), (32, 1)}
    for p in plans.values():
        assert p["target_tile"] == 256 and p["workgroup_size"] == 256
    # fewer targets than slots: M = 1 against every K > 1; (2, 1500, 37) is the widest cloud whose targets fit one
    # list (37 > 32, so K never exceeds its M: test_lengths_and_poisoned_padding cuts a wide cloud below K instead)
    for shape in ((1, 1, 1), (2, 300, 1)):
        assert shape in ref.SHAPES and shape[2] < min(K for K in kref.KS if K > 1)
    assert (2, 1500, 37) in ref.SHAPES


@pytest.mark.parametrize("K", kref.KS)
@pytest.mark.parametrize("k", CASES)
def test_knn_points_matches_the_restatement(k, K):
    x, y = _clouds(k)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    want, want_idx, gap_prev, gap_next = kref.knn(x, y, K, rows=kref.cached_sorted_rows(k))
    clear = kref.clear_slots(gap_prev, gap_next)
    unclear = int(((want_idx >= 0) & ~clear).sum())
    print("%s K=%d: %d unclear of %d slots" % (k, K, unclear, clear.numel()))
    assert unclear <= kref.UNCLEAR_CAP * clear.numel()          # before the comparison
    xd, yd = _on_device(k)
    xg, yg = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
    got, idx = points.knn_points(xg, yg, K)
    assert got.shape == idx.shape == (B, N, K) and got.dtype == torch.float32 and idx.dtype == torch.int32
    assert got.is_cuda and not idx.requires_grad and got.grad_fn is not None
    idx_host = idx.cpu()
    kept = min(K, M)
    assert bool((idx_host[..., :kept] >= 0).all()) and bool((idx_host[..., :kept] < M).all())
    assert bool((idx_host[..., kept:] == -1).all()) and bool((got[..., kept:] == 0).all())
    _close(got.detach(), want, 1e-6, "%s K=%d sqdist" % (k, K))
    _close(kref.distance_to(x, y, idx_host), want, 1e-6, "%s K=%d distance to the named neighbours" % (k, K))
    assert torch.equal(idx_host.long()[clear], want_idx[clear])
    # the K slots of a query name K different targets
    ordered = idx_host[..., :kept].long().sort(dim=-1).values
    assert kept == 1 or bool((ordered[..., 1:] != ordered[..., :-1]).all())
    upstream = torch.randn(got.shape, generator=torch.Generator().manual_seed(3))
    got.backward(upstream.to(DEV))
    wdx, wdy = kref.knn_gradients(x, y, idx_host, upstream)
    _grad_close(xg.grad, wdx, "%s K=%d dx" % (k, K))
    _grad_close(yg.grad, wdy, "%s K=%d dy" % (k, K))


@pytest.mark.parametrize("k", CASES)
def test_prefix_property(k):
    """The first K' columns of a K-neighbour call are the K'-neighbour call, bit for bit: neither the list capacity
    nor the launch shape (queries per lane, packed or scalar arithmetic, splits) reaches the result."""
    xd, yd = _on_device(k)
    with torch.no_grad():
        for K, fewer in ((32, 8), (16, 3), (8, 1)):
            whole, whole_idx = points.knn_points(xd, yd, K)
            part, part_idx = points.knn_points(xd, yd, fewer)
            assert torch.equal(whole[..., :fewer], part), (k, K, fewer)
            assert torch.equal(whole_idx[..., :fewer], part_idx), (k, K, fewer)


@pytest.mark.parametrize("k", CASES)
def test_one_neighbour_is_the_nearest_point(k):
    x, y = _clouds(k)
    xd, yd = _on_device(k)
    with torch.no_grad():
        got, idx = points.knn_points(xd, yd, 1)
        near, near_idx = points.nearest_points(xd, yd)
    _, _, gap = ref.nearest(x, y) if k == "translated" else ref.cached_nearest(k)
    clear = gap > ref.RUNNER_UP_MARGIN
    assert torch.equal(idx[..., 0].cpu()[clear], near_idx.cpu()[clear])
    _close(got[..., 0], near.double().cpu(), 1e-6, "%s K=1 against nearest_points" % (k,))


@pytest.mark.parametrize("wide", [False, True])
def test_exact_ties_go_to_the_lowest_index(wide):
    x, y = ref.lattice_clouds(wide)
    assert (_native.knn_plan(1, x.shape[1], y.shape[1], 16)["splits"] > 1) == wide
    for K in (5, 16, 20):     # sixteen targets at 0.75, then the ring at 2.75: 20 cuts through a tie group
        want, want_idx, _, _ = kref.knn(x, y, K)
        assert bool((want[..., :min(K, 16)] == 0.75).all()) and (K <= 16 or bool((want[..., 16:] == 2.75).all()))
        got, idx = points.knn_points(x.to(DEV), y.to(DEV), K)
        assert torch.equal(got.double().cpu(), want)      # exact in float32 under any contraction
        assert torch.equal(idx.cpu().long(), want_idx)


def test_self_query():
    x, _ = _on_device(8)       # (2, 1025, 3): seeded, without duplicates
    got, idx = points.knn_points(x, x, 4)
    assert bool((got[..., 0] == 0).all())
    assert torch.equal(idx[..., 0].cpu().long(), torch.arange(1025)[None].expand(2, -1))
    assert bool((got[..., 1] > 0).all())


def test_lengths_and_poisoned_padding():
    x, y = ref.clouds(4)                       # (2, 257, 1031): splits
    x, y = torch.cat([x, x[:1], x[1:]]), torch.cat([y, y[:1], y[1:]])   # four images
    xl, yl = torch.tensor([257, 100, 257, 257]), torch.tensor([1031, 300, 5, 0])
    K = 8
    assert _native.knn_plan(4, 257, 1031, K)["splits"] > 1
    want, want_idx, gap_prev, gap_next = kref.knn(x, y, K, xl, yl)
    clear = kref.clear_slots(gap_prev, gap_next)
    upstream = torch.randn(4, 257, K, generator=torch.Generator().manual_seed(5))
    runs = []
    for fill in (None, 1e30, float("nan")):
        cx, cy = x.clone(), y.clone()
        if fill is not None:
            for b in range(4):
                cx[b, int(xl[b]):] = fill
                cy[b, int(yl[b]):] = fill
        xg, yg = cx.to(DEV).requires_grad_(True), cy.to(DEV).requires_grad_(True)
        got, idx = points.knn_points(xg, yg, K, xl.to(DEV), yl.to(DEV))
        got.backward(upstream.to(DEV))
        runs.append((got.detach(), idx, xg.grad, yg.grad))
    for other in runs[1:]:                     # the padding influences nothing, bit for bit
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    got, idx, dx, dy = runs[0]
    assert torch.equal(idx.cpu().long()[clear], want_idx[clear])
    assert torch.equal(idx.cpu() < 0, want_idx < 0)
    _close(got, want, 1e-6, "padded sqdist")
    assert bool((idx[2, :, 5:] == -1).all()) and bool((got[2, :, 5:] == 0).all())
    assert bool((idx[2, :, :5] >= 0).all()) and bool((idx[2, :, :5] < 5).all())
    assert bool((idx[3] == -1).all()) and bool((got[3] == 0).all())
    assert bool((idx[1, 100:] == -1).all()) and bool((got[1, 100:] == 0).all()) and bool((idx[1, :100] < 300).all())
    wdx, wdy = kref.knn_gradients(x, y, idx.cpu(), upstream)
    _grad_close(dx, wdx, "padded dx")
    _grad_close(dy, wdy, "padded dy")
    assert bool((dx[1, 100:] == 0).all()) and bool((dx[3] == 0).all())
    assert bool((dy[1, 300:] == 0).all()) and bool((dy[2, 5:] == 0).all()) and bool((dy[3] == 0).all())
    # lengths beyond the clouds are clamped by the kernel, int64 lengths are taken
    over = points.knn_points(x.to(DEV), y.to(DEV), K, torch.tensor([9999, 257, 300, 257], device=DEV),
                             torch.tensor([1031, 2 ** 40, 5000, 1031], device=DEV))
    plain = points.knn_points(x.to(DEV), y.to(DEV), K)
    assert torch.equal(over[0], plain[0]) and torch.equal(over[1], plain[1])


@pytest.mark.parametrize("k", [3, 4])   # without and with a split
def test_a_nan_target_sorts_last(k):
    x, y = ref.clouds(k)
    M = y.shape[1]
    xd, yd = _on_device(k)
    clean, clean_idx = points.knn_points(xd, yd, 8)
    bad = y.clone()
    bad[0, 7, 2] = float("nan")
    xg, yg = xd.clone().requires_grad_(True), bad.to(DEV).requires_grad_(True)
    got, idx = points.knn_points(xg, yg, 8)
    assert bool((idx >= 0).all()) and bool((idx < M).all())
    assert bool((idx[0] != 7).all()) and bool(torch.isfinite(got).all())      # eight finite distances exist
    assert torch.equal(got[1:], clean[1:]) and torch.equal(idx[1:], clean_idx[1:])
    unaffected = (clean_idx[0] != 7).all(dim=-1)
    assert torch.equal(got[0][unaffected], clean[0][unaffected]) and torch.equal(idx[0][unaffected], clean_idx[0][unaffected])
    got.sum().backward()
    assert bool(torch.isfinite(xg.grad).all())
    # fewer than K finite distances: the NaN takes the last slot and reports +inf, without a gradient
    few = bad[:, :10].to(DEV).requires_grad_(True)
    xg = xd.clone().requires_grad_(True)
    got, idx = points.knn_points(xg, few, 10)
    assert bool((idx >= 0).all()) and bool((idx < 10).all())
    assert bool((idx[0, :, 9] == 7).all()) and bool((got[0, :, 9] == float("inf")).all())
    assert bool(torch.isfinite(got[0, :, :9]).all()) and bool(torch.isfinite(got[1:]).all())
    got.backward(torch.ones_like(got))
    assert bool(torch.isfinite(xg.grad).all()) and bool((few.grad[0, 7] == 0).all())


def test_bitwise_reproducible_in_either_mode():
    x, y = _on_device(4)
    upstream = torch.randn(2, 257, 16, generator=torch.Generator().manual_seed(6)).to(DEV)

    def run():
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        got, idx = points.knn_points(xg, yg, 16)
        got.backward(upstream)
        return got.detach(), idx, xg.grad, yg.grad

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


def test_captured_step_replays_to_the_eager_result():
    x, y = ref.clouds(4)
    v = x.to(DEV).requires_grad_(True)
    scan = y.to(DEV)
    lengths = torch.tensor([1031, 450], device=DEV)
    weights = torch.linspace(1.0, 0.25, 8, device=DEV)

    def loss_of(m):
        sqdist, _ = points.knn_points(m, scan, 8, y_lengths=lengths)
        return (sqdist * weights).sum() + points.knn_points(scan, m, 3, lengths)[0].sum()

    def step():
        loss = loss_of(v)
        loss.backward()
        return loss

    captured = mesh_renderer.capture_step(step, [v])
    with torch.no_grad():
        v.add_(0.05 * torch.randn(2, 257, 3, generator=torch.Generator().manual_seed(9)).to(DEV))
    loss = captured.replay().clone()
    grad = v.grad.clone()
    fresh = v.detach().clone().requires_grad_(True)
    eager = loss_of(fresh)
    eager.backward()
    assert torch.equal(loss, eager.detach()) and torch.equal(grad, fresh.grad)
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0


def test_unrequested_gradients_are_not_computed(monkeypatch):
    x, y = _on_device(3)
    built = []
    real = _native.nearest_inverted_index
    monkeypatch.setattr(_native, "nearest_inverted_index", lambda *a, **k: built.append(1) or real(*a, **k))
    xg, yd = x.clone().requires_grad_(True), y.clone()
    got, idx = points.knn_points(xg, yd, 8)
    got.sum().backward()
    assert yd.grad is None and xg.grad is not None and not built
    wdx, _ = kref.knn_gradients(*_clouds(3), idx.cpu(), torch.ones(got.shape))
    _grad_close(xg.grad, wdx, "dx alone")
    xd, yg = x.clone(), y.clone().requires_grad_(True)
    got, idx = points.knn_points(xd, yg, 8)
    got.sum().backward()
    assert xd.grad is None and len(built) == 1
    _, wdy = kref.knn_gradients(*_clouds(3), idx.cpu(), torch.ones(got.shape))
    _grad_close(yg.grad, wdy, "dy alone")
    assert points.knn_points(xd, y, 8)[0].grad_fn is None       # no gradient wanted: no backward node


def test_input_forms_and_return_nn():
    x, y = _on_device(3)
    wide = torch.zeros(3, 65, 6, device=DEV)
    wide[..., 1::2] = x
    view = wide[..., 1::2]
    assert not view.is_contiguous()
    plain, plain_idx = points.knn_points(x, y, 5)
    got, idx, nn = points.knn_points(view, y, 5, return_nn=True)
    assert torch.equal(got, plain) and torch.equal(idx, plain_idx)
    assert nn.shape == (3, 65, 5, 3) and torch.equal(nn, points.knn_gather(y, idx))
    assert torch.equal(((x[:, :, None, :] - nn) ** 2).sum(-1).cpu() > 0, got.cpu() > 0)
    d, i = points.knn_points(x[1], y[1], 5, y_lengths=torch.tensor([40], device=DEV, dtype=torch.int64))
    assert d.shape == (65, 5) and bool((i < 40).all())
    assert torch.equal(i, points.knn_points(x[1:2], y[1:2, :40], 5)[1][0])
    with pytest.raises(RuntimeError):
        points.knn_points(x, y.cpu(), 5)       # clouds on two devices
    with pytest.raises(RuntimeError):
        points.knn_points(x, y, 5, x_lengths=torch.tensor([1, 2, 3]))   # lengths on the host


def test_normals_on_the_device_equal_the_host_path():
    example = kref.load_example()
    cloud = example.ellipsoid_cloud(2000)
    sensor = torch.tensor(example.SENSOR)
    on_device = points.estimate_point_normals(cloud.to(DEV), K=16, orient_to=sensor.to(DEV))
    on_host = points.estimate_point_normals(cloud, K=16, orient_to=sensor)
    assert on_device.is_cuda and on_device.dtype == torch.float32 and on_device.shape == (2000, 3)
    idx_device = points.knn_points(cloud.to(DEV), cloud.to(DEV), 16)[1].cpu().long().sort(dim=-1).values
    idx_host = points.knn_points(cloud, cloud, 16)[1].long().sort(dim=-1).values
    same = (idx_device == idx_host).all(dim=-1)
    print("%d of 2000 neighbour sets identical" % int(same.sum()))
    assert int(same.sum()) >= 0.99 * 2000
    cosine = (on_device.cpu().double() * on_host.double()).sum(-1).abs()
    print("min |cos| over them %.9f" % float(cosine[same].min()))
    assert bool((cosine[same] >= 1 - 1e-6).all())
    towards = (on_device.cpu() * (sensor - cloud)).sum(-1)
    assert bool((towards >= -1e-6).all())
