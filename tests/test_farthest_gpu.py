"""mesh_renderer.points.sample_farthest_points on the MI355X (csrc/farthest.hip) against the restatement of its
definition (tests/farthest_reference.py).

The definition fixes every float32 operation and its order, so idx and radius are compared with fps32 for EQUALITY,
on both routes (the cloud in one workgroup's registers; one launch per step) and at every N at which the plan changes
its route, its workgroup size or its points per lane.  Independently of the float32 restatement, greedy_shortfall
holds the kernel's indices to the float64 definition at every step: the selected point is within
points_reference.RUNNER_UP_MARGIN (4e-6 relative: two correctly rounded float32 distances closer than this may swap)
of the farthest.  On the host fps32 has shortfall 0 on these clouds (tests/test_farthest_host.py); their smallest
float64 gap to the runner-up, 2.5e-6, is below the margin, which is why the float64 comparison is the shortfall and
not index equality.  K <= 256 everywhere: the per-step route is at most 257 small launches."""
import numpy as np
import pytest
import torch

import farthest_reference as fref
import points_reference as pref
from pytorch_mesh_renderer_amd import _native, mesh_renderer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
points = mesh_renderer.points
RESIDENT, STEPS = _native.FARTHEST_ROUTE_RESIDENT, _native.FARTHEST_ROUTE_STEPS
_device_clouds = {}


def _on_device(k):
    if k not in _device_clouds:
        _device_clouds[k] = fref.cloud(k).to(DEV)
    return _device_clouds[k]


def _shape_of(N):
    p = _native.farthest_plan(1, N, 16)
    return (1, p["workgroup_size"], p["points_per_lane"]) if p["route"] == 1 else (2,)


def _changes(lo, hi):
    """Every N in [lo, hi) whose launch shape differs from that of N + 1, by bisection."""
    if _shape_of(lo) == _shape_of(hi):
        return []
    if hi == lo + 1:
        return [lo]
    mid = (lo + hi) // 2
    return _changes(lo, mid) + _changes(mid, hi)


def _boundaries():
    marks = sorted({1} | {2 ** e for e in range(1, 18)} | {3 * 2 ** e for e in range(16)})
    return [n for lo, hi in zip(marks[:-1], marks[1:]) for n in _changes(lo, hi)]


def _equal(idx, radius, want_idx, want_radius, what):
    assert idx.dtype == torch.int32 and radius.dtype == torch.float32 and idx.is_cuda and radius.is_cuda, what
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), want_idx), what
    assert np.array_equal(radius.cpu().numpy(), want_radius), what


def test_the_shapes_cover_every_launch_path():
    bounds = _boundaries()
    last_resident = max(n for n in bounds if _shape_of(n)[0] == 1)
    assert _shape_of(last_resident + 1) == (2,) and last_resident <= 24576
    assert _native.farthest_plan(1, 1 << 20, 16)["route"] == 2           # and it stays with the per-step route
    listed = {_shape_of(N) for _, N in fref.SHAPES} | {_shape_of(fref.cloud("translated").shape[1])}
    assert (2,) in listed and any(s[0] == 1 for s in listed)
    sizes = {s[1] for n in bounds + [1] for s in [_shape_of(n)] if s[0] == 1}
    assert 64 in sizes                                                    # the one-wavefront case exists
    for size in sizes:                                                    # every workgroup size the plan ever takes
        assert any(s[0] == 1 and s[1] == size for s in listed), size


@pytest.mark.parametrize("k", fref.CASES)
def test_matches_the_definition(k):
    cloud = fref.cloud(k)
    B, N, _ = cloud.shape
    K = min(N, fref.MAX_K)
    want_idx, want_radius = fref.cached_fps32(k)
    sampled, idx, radius = points.sample_farthest_points(_on_device(k), K, return_radius=True)
    assert sampled.shape == (B, K, 3) and idx.shape == radius.shape == (B, K)
    _equal(idx, radius, want_idx, want_radius, k)
    assert torch.equal(sampled.cpu(), torch.gather(cloud, 1, idx.cpu().long()[..., None].expand(-1, -1, 3)))
    ordered = idx.cpu().long().sort(dim=1).values
    assert K == 1 or bool((ordered[:, 1:] != ordered[:, :-1]).all())
    assert bool(torch.isinf(radius[:, 0]).all()) and bool((radius[:, 2:] <= radius[:, 1:-1]).all())
    shortfall = fref.greedy_shortfall(cloud.numpy(), idx.cpu().numpy())
    print("%s: greedy shortfall %.3g" % (k, shortfall))
    assert shortfall <= pref.RUNNER_UP_MARGIN


@pytest.mark.parametrize("k", fref.CASES)
def test_both_routes_agree_bit_for_bit(k):
    cloud = _on_device(k)
    N = cloud.shape[1]
    K = min(N, fref.MAX_K)
    want_idx, want_radius = fref.cached_fps32(k)
    stepped = _native.farthest_forward(cloud, K, route=STEPS)
    _equal(*stepped, want_idx, want_radius, (k, "steps"))
    if N > 24576:
        with pytest.raises(ValueError):
            _native.farthest_forward(cloud, K, route=RESIDENT)
        return
    resident = _native.farthest_forward(cloud, K, route=RESIDENT)
    assert torch.equal(resident[0], stepped[0]) and torch.equal(resident[1], stepped[1])


def test_every_boundary_of_the_plan():
    """A cloud exactly at every N after which the route, the workgroup size or the points per lane change, and at
    N + 1, K = 16: the plan's route against fps32, and the other route wherever it can hold the cloud."""
    bounds = _boundaries()
    assert len(bounds) >= 3
    for n in bounds:
        for N in (n, n + 1):
            cloud = np.random.default_rng(400 + N).uniform(-1, 1, (1, N, 3)).astype(np.float32)
            want_idx, want_radius = fref.fps32(cloud, min(N, 16))
            on_device = torch.from_numpy(cloud).to(DEV)
            _, idx, radius = points.sample_farthest_points(on_device, min(N, 16), return_radius=True)
            _equal(idx, radius, want_idx, want_radius, (N, _shape_of(N)))
            for route in (RESIDENT, STEPS):
                if route == STEPS or N <= 24576:
                    _equal(*_native.farthest_forward(on_device, min(N, 16), route=route), want_idx, want_radius,
                           (N, route))


def test_every_resident_shape_gives_the_same_result():
    """Every instantiation of the one-workgroup kernel (workgroup size x points per lane), forced, on the largest
    listed cloud it holds."""
    try:
        for size in (64, 256, 1024):
            for per_lane in (4, 8, 16, 20, 24):
                k = max(i for i, (_, N) in enumerate(fref.SHAPES) if N <= size * per_lane)
                _native.debug_set_farthest_shape(size, per_lane)
                got = _native.farthest_forward(_on_device(k), min(fref.SHAPES[k][1], 64), route=RESIDENT)
                want_idx, want_radius = fref.cached_fps32(k)
                _equal(*got, want_idx[:, :64], want_radius[:, :64], (size, per_lane, k))
        _native.debug_set_farthest_shape(64, 4)
        with pytest.raises(ValueError):
            _native.farthest_forward(_on_device(4), 8, route=RESIDENT)       # 257 points do not fit 64 x 4
    finally:
        _native.debug_set_farthest_shape(0, 0)


def test_lengths_and_poisoned_padding():
    cloud = fref.cloud(4)                                        # (2, 257)
    cloud = torch.cat([cloud, cloud])                            # four clouds
    lengths = torch.tensor([257, 100, 1, 0])
    start = torch.tensor([256, 5000, -3, 7])                     # the last valid, beyond the length, negative, empty
    K = 120                                                      # above the lengths 100, 1 and 0
    want_idx, want_radius = fref.fps32(cloud.numpy(), K, lengths.numpy(), start.numpy())
    for route in (RESIDENT, STEPS):
        for fill in (None, 1e30, float("nan")):
            padded = cloud.clone()
            if fill is not None:
                for b in range(4):
                    padded[b, int(lengths[b]):] = fill
            got = _native.farthest_forward(padded.to(DEV), K, lengths.to(DEV).int(), start.to(DEV).int(), route=route)
            _equal(*got, want_idx, want_radius, (route, fill))
    sampled, idx, radius = points.sample_farthest_points(padded.to(DEV), K, lengths.to(DEV), start.to(DEV),
                                                         return_radius=True)
    _equal(idx, radius, want_idx, want_radius, "public")
    assert bool((sampled[idx < 0] == 0).all()) and bool(torch.isfinite(sampled).all())
    # the call on the cut cloud
    _, cut_idx, cut_radius = points.sample_farthest_points(cloud[1:2, :100].to(DEV), K,
                                                           start_idx=torch.tensor([99], device=DEV), return_radius=True)
    assert torch.equal(cut_idx[0], idx[1]) and torch.equal(cut_radius[0], radius[1])
    # lengths beyond the cloud are clamped by the kernel, int64 is taken
    over = points.sample_farthest_points(cloud.to(DEV), 9, torch.tensor([9999, 2 ** 40, 257, 257], device=DEV))
    assert torch.equal(over[1], points.sample_farthest_points(cloud.to(DEV), 9)[1])


def test_non_finite_points_are_selected_last_and_in_index_order():
    cloud = fref.cloud(3)[:1].clone()                            # (1, 65)
    bad = [4, 17, 40, 64]
    clean = np.delete(cloud.numpy(), bad, axis=1)
    cloud[0, 4, 0] = float("nan")
    cloud[0, 17, 1] = float("inf")
    cloud[0, 40] = float("-inf")
    cloud[0, 64, 2] = float("nan")
    want_idx, want_radius = fref.fps32(cloud.numpy(), 65)
    assert list(want_idx[0, 61:]) == bad
    kept = np.delete(np.arange(65), bad)
    for route in (RESIDENT, STEPS):
        idx, radius = _native.farthest_forward(cloud.to(DEV), 65, route=route)
        _equal(idx, radius, want_idx, want_radius, route)
        assert idx[0, 61:].tolist() == bad and bool((radius[0, 61:] == 0).all())
        clean_idx, clean_radius = _native.farthest_forward(torch.from_numpy(clean).to(DEV), 61, route=route)
        assert np.array_equal(idx[0, :61].cpu().numpy(), kept[clean_idx[0].cpu().numpy()])
        assert torch.equal(radius[0, :61], clean_radius[0])
        # a non-finite start moves nobody
        got = _native.farthest_forward(cloud.to(DEV), 3, None, torch.tensor([40], device=DEV, dtype=torch.int32), route)
        _equal(*got, *fref.fps32(cloud.numpy(), 3, None, [40]), (route, "start"))


def test_duplicates_are_taken_before_anything_repeats():
    rng = np.random.default_rng(13)
    which = rng.permutation(np.concatenate([np.arange(10), rng.integers(0, 10, 90)]))    # every position occurs
    cloud = rng.uniform(-1, 1, (10, 3)).astype(np.float32)[which]
    for route in (RESIDENT, STEPS):
        idx, radius = _native.farthest_forward(torch.from_numpy(cloud)[None].to(DEV), 100, route=route)
        assert sorted(idx[0].tolist()) == list(range(100))
        assert bool((radius[0, 10:] == 0).all()) and bool((radius[0, 1:10] > 0).all())
        _equal(idx, radius, *fref.fps32(cloud[None], 100), route)


def test_bitwise_reproducible_in_either_mode():
    cloud = _on_device(6)                                        # (2, 5000)
    upstream = torch.randn(2, 64, 3, generator=torch.Generator().manual_seed(6)).to(DEV)

    def run():
        c = cloud.clone().requires_grad_(True)
        sampled, idx, radius = points.sample_farthest_points(c, 64, return_radius=True)
        (sampled * upstream).sum().backward()
        return sampled.detach(), idx, radius, c.grad, *_native.farthest_forward(cloud, 64, route=STEPS)

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


@pytest.mark.parametrize("route", [RESIDENT, STEPS])
def test_captured_step_replays_to_the_eager_result(route):
    first, second = _on_device(4), fref.cloud(4).flip(1).contiguous().to(DEV)     # (2, 257)
    lengths = torch.tensor([257, 90], device=DEV, dtype=torch.int32)
    static = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _native.farthest_forward(static, 32, lengths, route=route)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx, radius = _native.farthest_forward(static, 32, lengths, route=route)
    static.copy_(second)
    graph.replay()
    eager = _native.farthest_forward(second, 32, lengths, route=route)
    assert torch.equal(idx, eager[0]) and torch.equal(radius, eager[1])
    assert not torch.equal(idx, _native.farthest_forward(first, 32, lengths, route=route)[0])


def test_captured_public_step_with_gradient():
    cloud = fref.cloud(4)
    v = cloud.to(DEV).requires_grad_(True)
    weights = torch.linspace(1.0, 0.25, 24, device=DEV)[None, :, None]

    def loss_of(c):
        sampled, _ = points.sample_farthest_points(c, 24)
        return (sampled * weights).sum()

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
    assert int((grad != 0).any(dim=-1).sum()) == 2 * 24


def test_input_forms():
    cloud = _on_device(3)                                        # (2, 65)
    wide = torch.zeros(2, 65, 6, device=DEV)
    wide[..., 1::2] = cloud
    view = wide[..., 1::2]
    assert not view.is_contiguous()
    plain = points.sample_farthest_points(cloud, 20, return_radius=True)
    got = points.sample_farthest_points(view, 20, return_radius=True)
    assert len(points.sample_farthest_points(cloud, 20)) == 2 and len(plain) == 3
    for a, b in zip(plain, got):
        assert torch.equal(a, b)
    one = points.sample_farthest_points(cloud[1], 20, torch.tensor(40, device=DEV), torch.tensor(3, device=DEV),
                                        return_radius=True)
    assert one[0].shape == (20, 3) and one[1].shape == one[2].shape == (20,) and int(one[1][0]) == 3
    assert torch.equal(one[1], points.sample_farthest_points(cloud[1:2, :40], 20, start_idx=torch.tensor([3], device=DEV))[1][0])
    with pytest.raises(RuntimeError):
        points.sample_farthest_points(cloud, 5, lengths=torch.tensor([1, 2]))     # lengths on the host
    # other dtypes take the torch loop on the device
    _, idx64, radius64 = points.sample_farthest_points(cloud.double(), 20, return_radius=True)
    assert radius64.dtype == torch.float64 and torch.equal(idx64, plain[1])


def test_gradient_of_sampled():
    cloud = fref.cloud(2)                                        # (3, 63)
    lengths = torch.tensor([63, 5, 0], device=DEV)
    c = cloud.to(DEV).requires_grad_(True)
    sampled, idx = points.sample_farthest_points(c, 8, lengths)
    assert sampled.grad_fn is not None and not idx.requires_grad
    upstream = torch.randn(3, 8, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    (sampled * upstream.float().to(DEV)).sum().backward()
    c64 = cloud.double().requires_grad_(True)
    at = idx.cpu().long()
    gathered = torch.gather(c64, 1, at.clamp(min=0)[..., None].expand(-1, -1, 3))
    (torch.where((at >= 0)[..., None], gathered, torch.zeros_like(gathered)) * upstream.float().double()).sum().backward()
    assert torch.equal(c.grad.cpu().double(), c64.grad)          # one term per point: nothing to round
    assert bool((c.grad[2] == 0).all()) and bool((idx[1, 5:] == -1).all())
