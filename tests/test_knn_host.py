"""mesh_renderer.points.knn_points / knn_gather / estimate_point_normals on the host: the chunked torch path against
the float64 restatement (tests/knn_reference.py), the argument checks, the mr_knn_* validation and launch plan, and
the count of slots whose index float32 cannot decide.

Budgets (the GPU tests' too, taken from tests/test_points_gpu.py): sqdist within 1e-6 relative of float64 (one
rounding each in the subtraction, the product and the two sums, below 4 * 2^-24); the float64 distance to each named
neighbour within 1e-6 relative of the true k-th distance; idx equal to the restatement in every slot whose gaps to
both adjacent neighbours exceed RUNNER_UP_MARGIN; gradients within 1e-4 of the largest magnitude of the expected
tensor, the restatement evaluated with the path's own indices.  In float64 the torch path IS the restatement's
expression: every index equal, values and gradients to 1e-12."""
import ctypes

import pytest
import torch

import knn_reference as kref
import points_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer

points = mesh_renderer.points
ALL_CLOUDS = list(range(len(ref.SHAPES))) + ["translated"]


def _clouds(k):
    return ref.translated_clouds() if k == "translated" else ref.clouds(k)


def test_the_functions_are_exported():
    for name in ("knn_points", "knn_gather", "estimate_point_normals"):
        assert callable(getattr(mesh_renderer.points, name))


@pytest.mark.parametrize("k", ALL_CLOUDS)
def test_unclear_slots_are_rare(k):
    """What the index comparisons rely on: at most 0.1 % of the slots of any (shape, K) have a neighbour within
    RUNNER_UP_MARGIN; K <= 8 has at most 2 of them on any shape."""
    x, y = _clouds(k)
    for K in kref.KS:
        _, idx, gap_prev, gap_next = kref.knn(x, y, K, rows=kref.cached_sorted_rows(k))
        unclear = int(((idx >= 0) & ~kref.clear_slots(gap_prev, gap_next)).sum())
        print("%s K=%d: %d unclear of %d slots" % (k, K, unclear, idx.numel()))
        assert unclear <= kref.UNCLEAR_CAP * idx.numel()
        assert K > 8 or unclear <= 2
    if k == 9:
        _, idx, gap_prev, gap_next = kref.knn(x, y, 32, rows=kref.cached_sorted_rows(k))
        assert idx.numel() == 32800 and int(((idx >= 0) & ~kref.clear_slots(gap_prev, gap_next)).sum()) == 12


@pytest.mark.parametrize("k", ALL_CLOUDS)
def test_torch_path_matches_the_restatement_in_float64(k):
    x, y = _clouds(k)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    for K in kref.KS:
        want, want_idx, _, _ = kref.knn(x, y, K, rows=kref.cached_sorted_rows(k))
        xg, yg = x.double().requires_grad_(True), y.double().requires_grad_(True)
        got, idx = points.knn_points(xg, yg, K)
        assert got.shape == idx.shape == (B, N, K) and got.dtype == torch.float64 and idx.dtype == torch.int32
        assert not idx.requires_grad and got.grad_fn is not None
        assert torch.equal(idx.long(), want_idx)
        assert bool((idx[..., min(K, M):] == -1).all()) and bool((got[..., min(K, M):] == 0).all())
        assert float((got.detach() - want).abs().max()) <= 1e-12 * max(1.0, float(want.max()))
        g = torch.Generator().manual_seed(3)
        upstream = torch.randn(got.shape, generator=g, dtype=torch.float64)
        got.backward(upstream)
        wdx, wdy = kref.knn_gradients(x, y, idx, upstream)
        assert float((xg.grad - wdx).abs().max()) <= 1e-12 * max(1.0, float(wdx.abs().max()))
        assert float((yg.grad - wdy).abs().max()) <= 1e-12 * max(1.0, float(wdy.abs().max()))


@pytest.mark.parametrize("k", ALL_CLOUDS)
def test_torch_path_in_float32_keeps_the_budgets(k):
    x, y = _clouds(k)
    for K in (3, 32):
        want, want_idx, gap_prev, gap_next = kref.knn(x, y, K, rows=kref.cached_sorted_rows(k))
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        got, idx = points.knn_points(xg, yg, K)
        assert got.dtype == torch.float32
        assert bool(((got.detach().double() - want).abs() <= 1e-6 * want).all())
        assert bool(((kref.distance_to(x, y, idx) - want).abs() <= 1e-6 * want).all())
        clear = kref.clear_slots(gap_prev, gap_next)
        assert torch.equal(idx.long()[clear], want_idx[clear])
        upstream = torch.randn(got.shape, generator=torch.Generator().manual_seed(3))
        got.backward(upstream)
        wdx, wdy = kref.knn_gradients(x, y, idx, upstream)
        assert float((xg.grad.double() - wdx).abs().max()) <= 1e-4 * float(wdx.abs().max())
        assert float((yg.grad.double() - wdy).abs().max()) <= 1e-4 * float(wdy.abs().max())


def test_prefix_property_chunking_and_return_nn(monkeypatch):
    x, y = ref.clouds(4)
    whole, whole_idx, nn = points.knn_points(x, y, 32, return_nn=True)
    assert nn.shape == (2, 257, 32, 3) and torch.equal(nn, points.knn_gather(y, whole_idx))
    for K in (8, 3, 1):
        d, i = points.knn_points(x, y, K)
        assert torch.equal(d, whole[..., :K]) and torch.equal(i, whole_idx[..., :K])
    one, one_idx = points.nearest_points(x, y)
    assert torch.equal(one_idx, whole_idx[..., 0]) and torch.equal(one, whole[..., 0])
    monkeypatch.setattr(points, "_CHUNK_BYTES", 7 * 2 * 1031 * 3 * 4)    # a few query rows at a time
    chunked, chunked_idx = points.knn_points(x, y, 32)
    assert torch.equal(chunked, whole) and torch.equal(chunked_idx, whole_idx)
    # nn is differentiable in y through the gather
    yg = y.clone().requires_grad_(True)
    points.knn_points(x, yg, 2, return_nn=True)[2].sum().backward()
    assert float(yg.grad.sum()) == 2 * 257 * 2 * 3


def test_exact_ties_go_to_the_lowest_index():
    for wide in (False, True):
        x, y = ref.lattice_clouds(wide)
        for K in (5, 16, 20):     # sixteen targets at 0.75, then the ring at 2.75: 20 cuts through a tie group
            want, want_idx, _, _ = kref.knn(x, y, K)
            assert bool((want[..., :min(K, 16)] == 0.75).all()) and (K <= 16 or bool((want[..., 16:] == 2.75).all()))
            got, idx = points.knn_points(x, y, K)
            assert torch.equal(got.double(), want) and torch.equal(idx.long(), want_idx)


def test_self_query_and_unbatched_forms():
    x, _ = ref.clouds(8)
    d, i = points.knn_points(x, x, 4)
    assert bool((d[..., 0] == 0).all()) and torch.equal(i[..., 0].long(), torch.arange(1025)[None].expand(2, -1))
    d1, i1 = points.knn_points(x[1], x[1], 4, y_lengths=torch.tensor(100))
    assert d1.shape == (1025, 4) and i1.shape == (1025, 4) and bool((i1 < 100).all())
    assert torch.equal(i1, points.knn_points(x[1:], x[1:, :100], 4)[1][0])


def test_lengths_and_padding():
    x, y = ref.clouds(3)           # (3, 65, 63)
    xl, yl = torch.tensor([65, 20, 65]), torch.tensor([63, 5, 0])
    want, want_idx, _, _ = kref.knn(x, y, 8, xl, yl)
    runs = []
    for fill in (None, 1e30, float("nan")):
        cx, cy = x.clone(), y.clone()
        if fill is not None:
            for b in range(3):
                cx[b, int(xl[b]):] = fill
                cy[b, int(yl[b]):] = fill
        xg, yg = cx.requires_grad_(True), cy.requires_grad_(True)
        got, idx = points.knn_points(xg, yg, 8, xl, yl)
        got.backward(torch.randn(got.shape, generator=torch.Generator().manual_seed(5)))
        runs.append((got.detach(), idx, xg.grad, yg.grad))
    for other in runs[1:]:          # the padding influences nothing, bit for bit
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    got, idx, dx, dy = runs[0]
    assert torch.equal(idx.long(), want_idx) and bool(((got.double() - want).abs() <= 1e-6 * want).all())
    assert bool((idx[1, :20, 5:] == -1).all()) and bool((got[1, :20, 5:] == 0).all()) and bool((idx[1, :20, :5] >= 0).all())
    assert bool((idx[1, 20:] == -1).all()) and bool((idx[2] == -1).all()) and bool((got[2] == 0).all())
    assert bool((dx[1, 20:] == 0).all()) and bool((dx[2] == 0).all()) and bool((dy[1, 5:] == 0).all())
    assert bool((dy[2] == 0).all()) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dy).all())


def test_a_nan_target_sorts_last():
    x, y = ref.clouds(3)
    bad = y.clone()
    bad[0, 7, 2] = float("nan")
    clean, clean_idx = points.knn_points(x, y, 8)
    got, idx = points.knn_points(x, bad, 8)
    assert bool((idx >= 0).all()) and bool((idx < 63).all()) and bool((idx[0] != 7).all())
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got[1:], clean[1:]) and torch.equal(idx[1:], clean_idx[1:])
    # fewer than K finite distances: the NaN takes the last slot and reports +inf, without a gradient
    xg, yg = x.clone().requires_grad_(True), bad[:, :10].clone().requires_grad_(True)
    got, idx = points.knn_points(xg, yg, 10)
    assert bool((idx[0, :, 9] == 7).all()) and bool((got[0, :, 9] == float("inf")).all())
    assert bool(torch.isfinite(got[0, :, :9]).all()) and bool(torch.isfinite(got[1:]).all())
    got[torch.isfinite(got)].sum().backward()
    assert bool(torch.isfinite(xg.grad).all()) and bool((yg.grad[0, 7] == 0).all())


def test_argument_errors():
    x, y = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    for K in (0, 33, -1, 2.0, "3", True, None):
        with pytest.raises(ValueError):
            points.knn_points(x, y, K)
    with pytest.raises(TypeError):
        points.knn_points([0.0, 0.0, 0.0], y, 2)
    with pytest.raises(ValueError):
        points.knn_points(x[..., :2], y, 2)
    with pytest.raises(ValueError):
        points.knn_points(x[0], y, 2)
    with pytest.raises(RuntimeError):
        points.knn_points(x, y.double(), 2)
    with pytest.raises(RuntimeError):
        points.knn_points(x, y, 2, x_lengths=torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError):
        points.knn_points(x, y, 2, y_lengths=torch.tensor([1, 2, 3]))
    with pytest.raises(TypeError):
        points.knn_gather(y, [[0]])
    with pytest.raises(RuntimeError):
        points.knn_gather(y, torch.zeros(2, 5, 2))
    with pytest.raises(ValueError):
        points.knn_gather(y, torch.zeros(3, 5, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        points.estimate_point_normals(x, K=4, orient_to=torch.zeros(4))
    with pytest.raises(TypeError):
        points.estimate_point_normals(x, K=4, orient_to=[0.0, 0.0, 1.0])
    with pytest.raises(ValueError):
        points.estimate_point_normals(x, K=40)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.knn_forward(x, y, 2)


def test_knn_gather_with_missing_neighbours():
    values = torch.arange(2 * 4 * 2, dtype=torch.float64).reshape(2, 4, 2).requires_grad_(True)
    idx = torch.tensor([[[0, 3, -1]], [[2, -1, -1]]], dtype=torch.int32)
    out = points.knn_gather(values, idx)
    assert out.shape == (2, 1, 3, 2)
    assert out[0, 0].tolist() == [[0.0, 1.0], [6.0, 7.0], [0.0, 0.0]] and out[1, 0].tolist() == [[12.0, 13.0], [0.0, 0.0], [0.0, 0.0]]
    out.sum().backward()
    want = torch.zeros(2, 4, 2, dtype=torch.float64)
    want[0, 0] = want[0, 3] = want[1, 2] = 1.0
    assert torch.equal(values.grad, want)
    assert torch.equal(points.knn_gather(values.detach()[0], idx[0].long()), out.detach()[0])


def test_knn_plan_facts():
    plans = {}
    for B, N, M in ref.SHAPES + [(8, 10000, 10000), (32, 2502, 20000), (1, 100000, 100000), (65535, 1, 1)]:
        for K in (1, 3, 4, 5, 8, 9, 16, 17, 32):
            plan = plans[(B, N, M, K)] = _native.knn_plan(B, N, M, K)
            assert plan["list_capacity"] == (4 if K <= 4 else 8 if K <= 8 else 16 if K <= 16 else 32)
            assert plan["queries_per_lane"] in (1, {4: 4, 8: 2, 16: 1, 32: 1}[plan["list_capacity"]])
            assert (plan["queries_per_lane"] > 1) == (plan["list_capacity"] <= 8 and
                                                      N >= 256 * {4: 4, 8: 2}.get(plan["list_capacity"], 1))
            assert plan["target_tile"] == 256 and plan["workgroup_size"] == 256
            assert 1 <= plan["splits"] <= -(-M // 256)
            ws = _native.lib().mr_knn_workspace_bytes(B, N, M, K)
            assert ws == (0 if plan["splits"] == 1 else -(-(B * plan["splits"] * N * K * 8) // 256) * 256)
    assert plans[(1, 40, 5000, 8)]["splits"] > 1 and plans[(1, 1, 1, 8)]["splits"] == 1
    # the same fill heuristic as the K = 1 search where the queries per lane agree
    assert plans[(1, 40, 5000, 1)]["splits"] == _native.nearest_plan(1, 40, 5000)["splits"]
    for bad in ((0, 4, 4, 1), (1, 4, 4, 0), (1, 4, 4, 33), (1, 4, (1 << 28) + 1, 1), (1, 1 << 28, 4, 8),
                (65535, 1 << 20, 4, 2)):
        with pytest.raises(ValueError):
            _native.knn_plan(*bad)


def test_abi_validates_before_touching_a_device():
    L = _native.lib()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)   # never dereferenced: the calls below are rejected first
    assert L.mr_knn_workspace_bytes(1, 4, 4, 0) == 0 and L.mr_knn_workspace_bytes(1, 4, 4, 33) == 0
    assert L.mr_knn_workspace_bytes(0, 4, 4, 1) == 0 and L.mr_knn_workspace_bytes(1, 1 << 28, 4, 8) == 0
    assert L.mr_knn_workspace_bytes(1, 40, 5000, 8) == 20 * 40 * 8 * 8
    forward = lambda B, N, M, K, ws, have: L.mr_knn_forward(one, one, null, null, B, N, M, K, one, one, ws, have, null)
    for B, N, M, K in ((1, 4, 4, 0), (1, 4, 4, 33), (70000, 4, 4, 1), (1, 4, 0, 1), (1, 1 << 28, 4, 8),
                       (65535, 1 << 20, 4, 2)):
        assert forward(B, N, M, K, one, 1 << 30) == _native.MR_EINVAL
    assert L.mr_knn_forward(null, one, null, null, 1, 4, 4, 2, one, one, null, 0, null) == _native.MR_EINVAL
    assert L.mr_knn_forward(one, one, null, null, 1, 4, 4, 2, null, one, null, 0, null) == _native.MR_EINVAL
    assert forward(1, 40, 5000, 8, null, 0) == _native.MR_EWORKSPACE
    assert forward(1, 40, 5000, 8, one, 20 * 40 * 8 * 8 - 1) == _native.MR_EWORKSPACE
    assert forward(1, 40, 5000, 8, ctypes.c_void_p(264), 1 << 20) == _native.MR_EWORKSPACE     # misaligned
    backward = lambda K, *a: L.mr_knn_backward(one, one, null, null, 1, 4, 4, K, *a, null)
    assert backward(0, one, one, one, one, one, one, one) == _native.MR_EINVAL
    assert backward(33, one, one, one, one, one, one, one) == _native.MR_EINVAL
    assert backward(2, null, one, one, one, one, one, one) == _native.MR_EINVAL        # no saved distances
    assert backward(2, one, one, one, null, one, one, one) == _native.MR_EINVAL        # half an inverted index
    assert backward(2, one, one, null, null, one, one, one) == _native.MR_EINVAL       # dy without its index
    assert backward(2, one, one, null, null, null, one, null) == _native.MR_EINVAL     # no upstream


# ---- normals --------------------------------------------------------------------------------------------------------

def _eigh_normals(cloud, idx):
    """The restatement: torch.linalg.eigh in float64 on the host over the GIVEN neighbour indices -> (normals [N,3],
    eigenvalues [N,3] ascending)."""
    near = cloud.double()[idx.long()]                                   # [N,K,3]
    centred = near - near.mean(1, keepdim=True)
    covariance = centred.transpose(1, 2) @ centred / idx.shape[1]
    values, vectors = torch.linalg.eigh(covariance)
    return vectors[..., 0], values


def test_normals_match_eigh_on_the_examples_cloud():
    example = kref.load_example()
    cloud = example.ellipsoid_cloud(2000)
    for dtype in (torch.float32, torch.float64):
        normals = points.estimate_point_normals(cloud.to(dtype), K=16)
        assert normals.shape == (2000, 3) and normals.dtype == dtype and not normals.requires_grad
        _, idx = points.knn_points(cloud.to(dtype), cloud.to(dtype), 16)
        want, values = _eigh_normals(cloud, idx)
        decided = (values[:, 1] - values[:, 0]) / values[:, 2] > 1e-3
        assert int(decided.sum()) >= 1900
        cosine = (normals.double() * want).sum(-1).abs()
        print("%s: min |cos| %.9f over %d decided points" % (dtype, float(cosine[decided].min()), int(decided.sum())))
        assert bool((cosine[decided] >= 1 - 1e-6).all())
        assert bool(((normals.double().norm(dim=-1) - 1).abs() <= 1e-6).all())
    # batched equals unbatched, and a requires_grad cloud gives a result without a graph
    both = points.estimate_point_normals(torch.stack([cloud, cloud]).requires_grad_(True), K=16)
    alone = points.estimate_point_normals(cloud, K=16)
    assert not both.requires_grad and torch.equal(both[0], alone) and torch.equal(both[1], alone)


def test_a_plane_returns_its_normal_and_both_sign_rules():
    g = torch.Generator().manual_seed(2)
    uv = torch.rand(400, 2, generator=g, dtype=torch.float64)
    normal = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)
    normal = normal / normal.norm()
    e0 = torch.linalg.cross(normal, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
    e0 = e0 / e0.norm()
    e1 = torch.linalg.cross(normal, e0)
    cloud = uv[:, :1] * e0 + uv[:, 1:] * e1 + torch.tensor([0.3, 0.2, -0.1], dtype=torch.float64)
    got = points.estimate_point_normals(cloud, K=12)
    assert float((got - (-normal)).abs().max()) <= 1e-6        # the largest component, y, is made positive
    assert bool((got[:, 1] > 0).all())
    above = cloud.mean(0) + 3.0 * normal
    assert float((points.estimate_point_normals(cloud, K=12, orient_to=above) - normal).abs().max()) <= 1e-6
    below = torch.stack([cloud.mean(0) - 3.0 * normal, above])
    batch = points.estimate_point_normals(torch.stack([cloud, cloud]), K=12, orient_to=below)
    assert float((batch[0] + normal).abs().max()) <= 1e-6 and float((batch[1] - normal).abs().max()) <= 1e-6
    single = points.estimate_point_normals(cloud.float(), K=12, orient_to=above.float())
    assert single.dtype == torch.float32 and float((single.double() - normal).abs().max()) <= 1e-6
    # equal magnitudes: the lowest axis decides
    diagonal = torch.tensor([[1.0, -1.0, 0.0], [-1.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, -1.0, 1.0]],
                            dtype=torch.float64)     # the plane x + y = 0
    tie = points.estimate_point_normals(diagonal, K=5)
    assert bool((tie[:, 0] > 0).all()) and float((tie[:, :2] - 0.5 ** 0.5).abs().max()) <= 1e-9


def test_degenerate_neighbourhoods_get_the_zero_vector():
    two = torch.tensor([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    assert bool((points.estimate_point_normals(two, K=4) == 0).all())
    line = torch.linspace(0, 1, 9, dtype=torch.float64)[:, None] * torch.tensor([1.0, 2.0, -1.0], dtype=torch.float64)
    assert bool((points.estimate_point_normals(line, K=5) == 0).all())
    assert bool((points.estimate_point_normals(torch.zeros(6, 3), K=3) == 0).all())      # one point six times
    # padded rows, and an image with two valid points
    g = torch.Generator().manual_seed(4)
    cloud = torch.rand(2, 50, 3, generator=g)
    got = points.estimate_point_normals(cloud, K=6, lengths=torch.tensor([30, 2]))
    assert bool((got[0, 30:] == 0).all()) and bool((got[1] == 0).all())
    assert bool(((got[0, :30].norm(dim=-1) - 1).abs() <= 1e-6).all())
    assert torch.equal(got[0, :30], points.estimate_point_normals(cloud[0, :30], K=6))
