"""mesh_renderer.points.sample_farthest_points on the host: the torch loop against the restatement of the definition
(tests/farthest_reference.py) -- bit for bit against fps32 in float32 and against fps64 in float64 --, the argument
checks, lengths / start_idx / empty slots, the non-finite rule, exact ties, the gradient of `sampled`, and the
mr_farthest_* validation and launch plan.

No tolerance appears: the definition fixes every operation and its order, so indices and radii are compared for
equality.  What the GPU tests rely on is checked here too: on every shared cloud fps32 selects what fps64 selects and
is greedy in float64 at every step (greedy_shortfall 0)."""
import ctypes

import numpy as np
import pytest
import torch

import farthest_reference as fref
from pytorch_mesh_renderer_amd import _native, mesh_renderer

points = mesh_renderer.points


def _same(got_idx, got_radius, want_idx, want_radius):
    assert got_idx.dtype == torch.int32
    assert np.array_equal(got_idx.numpy().astype(np.int64), want_idx)
    assert got_radius.numpy().dtype == want_radius.dtype
    assert np.array_equal(got_radius.numpy(), want_radius)      # +inf == +inf; no NaN is ever a radius


def test_the_function_is_exported():
    assert callable(mesh_renderer.points.sample_farthest_points)


@pytest.mark.parametrize("k", fref.CASES)
def test_torch_path_matches_the_restatement(k):
    cloud = fref.cloud(k)
    B, N, _ = cloud.shape
    K = min(N, fref.MAX_K)
    want_idx, want_radius = fref.cached_fps32(k)
    sampled, idx, radius = points.sample_farthest_points(cloud, K, return_radius=True)
    assert sampled.shape == (B, K, 3) and idx.shape == radius.shape == (B, K) and sampled.dtype == torch.float32
    _same(idx, radius, want_idx, want_radius)
    assert torch.equal(sampled, torch.gather(cloud, 1, idx.long()[..., None].expand(-1, -1, 3)))
    ordered = np.sort(want_idx, axis=1)
    assert K == 1 or bool((ordered[:, 1:] != ordered[:, :-1]).all())
    assert bool(np.isinf(want_radius[:, 0]).all()) and bool((np.diff(want_radius[:, 1:], axis=1) <= 0).all())
    idx64, radius64 = fref.fps64(cloud.numpy(), K)
    _, got_idx, got_radius = points.sample_farthest_points(cloud.double(), K, return_radius=True)
    _same(got_idx, got_radius, idx64, radius64)
    # what the GPU tests lean on: float32 decides every step of these clouds as float64 does
    assert np.array_equal(want_idx, idx64)
    assert fref.greedy_shortfall(cloud.numpy(), want_idx) == 0.0


def test_argument_errors():
    cloud = fref.cloud(3)
    with pytest.raises(TypeError):
        points.sample_farthest_points(cloud.numpy(), 4)
    with pytest.raises(TypeError):
        points.sample_farthest_points(cloud.long(), 4)
    for bad in (cloud[..., :2], cloud[0, 0], cloud[:, :0]):
        with pytest.raises(ValueError):
            points.sample_farthest_points(bad, 4)
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            points.sample_farthest_points(cloud, bad)
    for name in ("lengths", "start_idx"):
        with pytest.raises(TypeError):
            points.sample_farthest_points(cloud, 4, **{name: [1, 2]})
        with pytest.raises(RuntimeError):
            points.sample_farthest_points(cloud, 4, **{name: torch.tensor([1.0, 2.0])})
        with pytest.raises(ValueError):
            points.sample_farthest_points(cloud, 4, **{name: torch.tensor([1, 2, 3])})


def test_lengths_start_idx_and_empty_slots():
    cloud = fref.cloud(4)                                        # (2, 257)
    cloud = torch.cat([cloud, cloud])                            # four clouds
    lengths = torch.tensor([257, 100, 1, 0])
    start = torch.tensor([256, 5000, -3, 7])                     # the last valid, beyond the length, negative, empty
    K = 120
    want_idx, want_radius = fref.fps32(cloud.numpy(), K, lengths.numpy(), start.numpy())
    assert want_idx[0, 0] == 256 and want_idx[1, 0] == 99 and want_idx[2, 0] == 0
    assert bool((want_idx[1, 100:] == -1).all()) and bool((want_idx[2, 1:] == -1).all()) and bool((want_idx[3] == -1).all())
    for fill in (None, 1e30, float("nan")):
        padded = cloud.clone()
        if fill is not None:
            for b in range(4):
                padded[b, int(lengths[b]):] = fill
        sampled, idx, radius = points.sample_farthest_points(padded, K, lengths, start, return_radius=True)
        _same(idx, radius, want_idx, want_radius)
        assert bool((sampled[idx < 0] == 0).all()) and bool((radius[idx < 0] == 0).all())
    # the call on the cut cloud
    _, cut_idx, cut_radius = points.sample_farthest_points(cloud[1:2, :100], K, start_idx=torch.tensor([99]),
                                                           return_radius=True)
    assert torch.equal(cut_idx[0], idx[1]) and torch.equal(cut_radius[0], radius[1])
    # lengths beyond the cloud are clamped, int64 is taken, a cloud without the batch axis takes 0-dim tensors
    over = points.sample_farthest_points(cloud, 9, torch.tensor([9999, 2 ** 40, 257, 257]))
    assert torch.equal(over[1], points.sample_farthest_points(cloud, 9)[1])
    one = points.sample_farthest_points(cloud[0], 9, torch.tensor(100), torch.tensor(3), return_radius=True)
    assert one[0].shape == (9, 3) and one[1].shape == one[2].shape == (9,) and int(one[1][0]) == 3
    assert bool((one[1] < 100).all())


def test_non_finite_points_are_selected_last_and_in_index_order():
    cloud = fref.cloud(3)[:1].clone()                            # (1, 65)
    bad = [4, 17, 40, 64]
    clean = np.delete(cloud.numpy(), bad, axis=1)
    cloud[0, 4, 0] = float("nan")
    cloud[0, 17, 1] = float("inf")
    cloud[0, 40] = float("-inf")
    cloud[0, 64, 2] = float("nan")
    want_idx, want_radius = fref.fps32(cloud.numpy(), 65)
    assert list(want_idx[0, 61:]) == bad and bool((want_radius[0, 61:] == 0).all())
    kept = np.delete(np.arange(65), bad)
    clean_idx, clean_radius = fref.fps32(clean, 61)
    assert np.array_equal(want_idx[0, :61], kept[clean_idx[0]]) and np.array_equal(want_radius[0, :61], clean_radius[0])
    for dtype, restated in ((torch.float32, fref.fps32), (torch.float64, fref.fps64)):
        _, idx, radius = points.sample_farthest_points(cloud.to(dtype), 65, return_radius=True)
        _same(idx, radius, *restated(cloud.numpy(), 65))
    # a non-finite start moves nobody: the next point is the lowest finite index, at +inf
    _, idx, radius = points.sample_farthest_points(cloud, 3, start_idx=torch.tensor([40]), return_radius=True)
    _same(idx, radius, *fref.fps32(cloud.numpy(), 3, None, [40]))
    assert idx[0].tolist()[:2] == [40, 0] and bool(torch.isinf(radius[0, :2]).all())


def test_exact_ties_go_to_the_lowest_index():
    """An 8 x 8 x 8 integer grid: every distance is exact in either precision, so every tie is decided by the index
    alone and float32 and float64 must agree."""
    grid = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(1, -1, 3)
    grid = grid[:, np.random.default_rng(12).permutation(512)].astype(np.float32)
    idx32, radius32 = fref.fps32(grid, 512)
    idx64, radius64 = fref.fps64(grid, 512)
    assert np.array_equal(idx32, idx64) and np.array_equal(radius32.astype(np.float64), radius64)
    assert sorted(idx32[0].tolist()) == list(range(512))
    assert len(np.unique(radius32[0, 1:])) < 30                  # ties everywhere
    _, idx, radius = points.sample_farthest_points(torch.from_numpy(grid), 512, return_radius=True)
    _same(idx, radius, idx32, radius32)


def test_duplicates_are_taken_before_anything_repeats():
    rng = np.random.default_rng(13)
    which = rng.permutation(np.concatenate([np.arange(10), rng.integers(0, 10, 90)]))    # every position occurs
    cloud = rng.uniform(-1, 1, (10, 3)).astype(np.float32)[which]
    distinct = 10
    _, idx, radius = points.sample_farthest_points(torch.from_numpy(cloud), 100, return_radius=True)
    assert sorted(idx.tolist()) == list(range(100))
    assert bool((radius[distinct:] == 0).all()) and bool((radius[1:distinct] > 0).all())
    _same(idx[None], radius[None], *fref.fps32(cloud[None], 100))


def test_gradient_of_sampled():
    cloud = fref.cloud(2).double().requires_grad_(True)          # (3, 63)
    lengths = torch.tensor([63, 5, 0])
    sampled, idx = points.sample_farthest_points(cloud, 8, lengths)
    assert sampled.grad_fn is not None and not idx.requires_grad
    upstream = torch.randn(3, 8, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    (sampled * upstream).sum().backward()
    want = torch.zeros(3, 63, 3, dtype=torch.float64)
    for b in range(3):
        for k in range(8):
            if idx[b, k] >= 0:
                want[b, idx[b, k]] += upstream[b, k]
    assert torch.equal(cloud.grad, want)
    assert bool((cloud.grad[2] == 0).all()) and bool((idx[1, 5:] == -1).all()) and bool((sampled[1, 5:] == 0).all())


def test_native_validation_without_a_gpu():
    L = _native.lib()
    out = (ctypes.c_int * 4)()
    slots = [ctypes.c_void_p(ctypes.addressof(out) + 4 * k) for k in range(4)]
    ok = [(1, 1, 1), (65535, 1, 1), (1, (1 << 28) - 1, 1), (1, 5, (1 << 24) - 1), (127, 9, (1 << 24) - 1)]
    bad = [(0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, 1 << 28, 1), (1, 5, 0), (1, 5, 1 << 24), (128, 9, 1 << 24),
           (129, 9, (1 << 24) - 1)]
    for dims in ok:
        assert L.mr_farthest_plan(*dims, *slots) == _native.MR_OK, dims
        assert L.mr_farthest_workspace_bytes(*dims) >= 256
    assert L.mr_farthest_plan(65535, 9, 32767, *slots) == _native.MR_OK          # B K < 2^31
    assert L.mr_farthest_plan(65535, 9, 32769, *slots) == _native.MR_EINVAL      # B K >= 2^31
    for dims in bad:
        assert L.mr_farthest_plan(*dims, *slots) == _native.MR_EINVAL, dims
        assert L.mr_farthest_workspace_bytes(*dims) == 0
        assert L.mr_farthest_forward(None, None, None, *dims, 0, None, None, None, 0, None) == _native.MR_EINVAL
        with pytest.raises(ValueError):
            _native.farthest_plan(*dims)
    assert L.mr_farthest_plan(1, 5, 5, None, *slots[1:]) == _native.MR_EINVAL
    assert L.mr_farthest_forward(None, None, None, 1, 5, 5, 0, None, None, None, 0, None) == _native.MR_EINVAL
    assert L.mr_debug_set_farthest_shape(128, 4) == _native.MR_EINVAL
    assert L.mr_debug_set_farthest_shape(64, 4) == _native.MR_OK and L.mr_debug_set_farthest_shape(0, 0) == _native.MR_OK
    # the wrappers refuse before anything reaches the library
    cloud = torch.zeros(2, 9, 3)
    with pytest.raises(ValueError):
        _native.farthest_forward(cloud, 1 << 24)
    with pytest.raises(ValueError):
        _native.farthest_forward(cloud, 0)
    with pytest.raises(RuntimeError):
        _native.farthest_forward(cloud.double(), 3)
    with pytest.raises(RuntimeError):
        _native.farthest_forward(cloud, 3, lengths=torch.tensor([1, 2]))          # int64: the public function converts
    with pytest.raises(ValueError):
        _native.farthest_forward(cloud, 3, route=3)
    with pytest.raises(RuntimeError, match="MI355X"):
        _native.farthest_forward(cloud, 3)                                        # no CPU fallback in the library


def test_the_plan():
    """Route 1 holds the cloud in one workgroup: its shape holds N and is the smallest that does; route 2 covers the
    cloud with its slices; the plan depends on N alone."""
    last = None
    for N in (1, 64, 256, 257, 1024, 1025, 4096, 4097, 16384, 16385, 24576, 24577, 40000, 10 ** 6, (1 << 28) - 1):
        p = _native.farthest_plan(1, N, 16)
        assert p == _native.farthest_plan(7, N, 200)
        assert p["route"] in (1, 2) and p["workgroup_size"] in (64, 256, 1024)
        if p["route"] == 1:
            assert p["slices"] == 1 and p["workgroup_size"] * p["points_per_lane"] >= N
            assert last is None or last["route"] == 1           # one crossover: route 1 below it, route 2 above
        else:
            assert p["workgroup_size"] == 256 and 1 <= p["slices"] <= 1024
            assert p["slices"] * p["points_per_lane"] * 256 >= N
            assert (p["slices"] - 1) * p["points_per_lane"] * 256 < N + 256 * p["slices"]
        last = p
    assert _native.farthest_plan(1, 1, 1)["route"] == 1 and _native.farthest_plan(1, (1 << 28) - 1, 1)["route"] == 2
