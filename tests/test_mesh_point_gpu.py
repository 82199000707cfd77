"""mesh_renderer.points.triangle_nearest_points / mesh_point_distance / point_mesh_face_distance on the MI355X (the
k_tp_* kernels of csrc/nearest.hip) against the float64 restatement (tests/mesh_point_reference.py).

Forward bound: mp.HIP_BOUND_UNITS = 4 x the worst error of the package's float32 torch path on the CPU (2.25, so 9.0)
in units of 2^-24 * scale, scale = max_k |p_j - v_k|^2 over the corners of the named pair, for |sqdist - min|, for
the float64 distance of the named pair above the minimum, and (twice the bound) for the float64 distance at the
returned barycentrics; an index equals the restatement's wherever its minimum is separated from the runner-up by
more than the bound.  Gradients: within 1e-4 of the largest magnitude of the expected gradient tensor, the
restatement evaluated with the returned (index, bary)."""
import pytest
import torch

import mesh_point_reference as mp
import point_mesh_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
points = mesh_renderer.points
reg = mesh_renderer.regularizers


def _grad_close(got, want, what):
    scale = float(want.abs().max())
    err = float((got.double().cpu() - want).abs().max())
    print("%s: gradient max err %.3g of scale %.3g" % (what, err, scale))
    assert err <= 1e-4 * scale, "%s: gradient error %.3g > 1e-4 * %.3g" % (what, err, scale)


def _dev(t):
    return None if t is None else t.to(DEV)


def _check(p, v, tri, out, what, lengths=None, in_unit_cube=True):
    sqdist, index, bary = out
    B, T = p.shape[0], tri.shape[0]
    assert sqdist.shape == index.shape == (B, T) and bary.shape == (B, T, 3)
    assert sqdist.dtype == bary.dtype == torch.float32 and index.dtype == torch.int32
    assert sqdist.is_cuda and index.is_cuda and bary.is_cuda and not index.requires_grad and not bary.requires_grad
    errors = mp.forward_errors(p, v, tri, sqdist, index, bary, lengths, mp.HIP_BOUND_UNITS)
    mp.check_forward(errors, mp.HIP_BOUND_UNITS, what, in_unit_cube)


@pytest.mark.parametrize("c", mp.CASES, ids=mp.name)
def test_triangle_nearest_points_matches_the_restatement(c):
    p, v, tri, lengths = mp.case(c)
    td, ld = tri.to(DEV), _dev(lengths)
    pg, vg = p.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    sqdist, index, bary = points.triangle_nearest_points(pg, vg, td, ld)
    assert sqdist.grad_fn is not None
    _check(p, v, tri, (sqdist, index, bary), mp.name(c), lengths, in_unit_cube=c[1] != "translated")
    g = torch.Generator().manual_seed(3)
    upstream = torch.randn(sqdist.shape, generator=g)
    sqdist.backward(upstream.to(DEV))
    wdp, wdv = mp.gradients(p, v, tri, index.cpu(), bary.cpu(), upstream)
    _grad_close(pg.grad, wdp, "%s dpoints" % mp.name(c))
    _grad_close(vg.grad, wdv, "%s dvertices" % mp.name(c))
    # each gradient alone
    alone = p.to(DEV).requires_grad_(True)
    points.triangle_nearest_points(alone, v.to(DEV), td, ld)[0].backward(upstream.to(DEV))
    assert torch.equal(alone.grad, pg.grad)
    alone = v.to(DEV).requires_grad_(True)
    points.triangle_nearest_points(p.to(DEV), alone, td, ld)[0].backward(upstream.to(DEV))
    assert torch.equal(alone.grad, vg.grad)


@pytest.mark.parametrize("c", mp.CASES, ids=mp.name)
def test_mesh_point_distance_matches_the_restatement(c):
    p, v, tri, lengths = mp.case(c)
    td, ld = tri.to(DEV), _dev(lengths)
    want, want_index, _ = mp.cached_nearest(c)
    pg, vg = p.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    mean = points.mesh_point_distance(pg, vg, td, ld)
    assert mean.shape == (p.shape[0],) and mean.dtype == torch.float32 and mean.is_cuda
    want_mean = mp.mean_of(want, v, tri)
    atol = mp.mean_atol(p, v, tri, want_index, mp.HIP_BOUND_UNITS)
    err = (mean.detach().double().cpu() - want_mean).abs()
    print("%s mean: worst err %.3g of %.3g" % (mp.name(c), float(err.max()), float(want_mean.max())))
    assert bool((err <= 1e-5 * want_mean + atol).all())
    g = torch.Generator().manual_seed(4)
    upstream = torch.randn(p.shape[0], generator=g)
    mean.backward(upstream.to(DEV))
    _, index, bary = points.triangle_nearest_points(p.to(DEV), v.to(DEV), td, ld)   # what the same kernels gave the loss
    wdp, wdv = mp.mean_gradients(p, v, tri, index.cpu(), bary.cpu(), upstream)
    _grad_close(pg.grad, wdp, "%s mean dpoints" % mp.name(c))
    _grad_close(vg.grad, wdv, "%s mean dvertices" % mp.name(c))
    alone = v.to(DEV).requires_grad_(True)
    points.mesh_point_distance(p.to(DEV), alone, td, ld).backward(upstream.to(DEV))
    assert torch.equal(alone.grad, vg.grad)
    alone = p.to(DEV).requires_grad_(True)
    points.mesh_point_distance(alone, v.to(DEV), td, ld).backward(upstream.to(DEV))
    assert torch.equal(alone.grad, pg.grad)


def test_thin_triangles_stay_between_the_minimum_and_the_nearest_edge():
    p, v, tri = ref.sliver_mesh()
    sqdist, index, bary = points.triangle_nearest_points(p.to(DEV), v.to(DEV), tri.to(DEV))
    mp.check_sliver(p, v, tri, sqdist, index, bary, mp.HIP_BOUND_UNITS, "thin triangles")


# (case, [(j, j')]): the point some triangle is nearest to is moved to row j and copied to row j' > j
TIES = [(("own", 3), [(10, 200), (300, 812), (600, 601)]),   # inside one tile, across a split boundary, a packed pair
        (("own", 4), [(10, 200), (100, 101)]),               # packed without a split: inside the tile, a pair
        (("own", 5), [(10, 150)])]                           # one point a step


@pytest.mark.parametrize("c,moves", TIES, ids=[mp.name(c) for c, _ in TIES])
def test_exact_ties_go_to_the_lowest_point(c, moves):
    p, v, tri, _ = mp.case(c)
    plan = _native.nearest_point_of_triangle_plan(1, p.shape[1], tri.shape[0])
    if c == ("own", 3):
        chunk = -(-(-(-p.shape[1] // plan["point_tile"])) // plan["splits"]) * plan["point_tile"]
        assert chunk == 256 and plan["points_per_step"] == 2    # rows 10 / 200 share a tile, 300 / 812 lie in two splits
    _, first, _ = mp.cached_nearest(c)
    chosen = [int(j) for j in first[0].unique()]
    assert len(chosen) >= len(moves)
    reserved = {j for pair in moves for j in pair}
    assert not reserved & set(chosen)
    q = p.clone()
    for (j, copy), source in zip(moves, chosen):
        q[0, j], q[0, source] = p[0, source], p[0, j]
        q[0, copy] = q[0, j]
    want, want_index, _ = mp.nearest(q, v, tri)
    concerned = torch.zeros(tri.shape[0], dtype=torch.bool)
    for j, copy in moves:                       # the restatement alone names the lower row of every copied pair
        assert bool((want_index[0] == j).any()) and not bool((want_index[0] == copy).any())
        concerned |= want_index[0] == j
    out = points.triangle_nearest_points(q.to(DEV), v.to(DEV), tri.to(DEV))
    _check(q, v, tri, out, "ties %s" % mp.name(c))
    index = out[1].cpu().long()
    assert torch.equal(index[0][concerned], want_index[0][concerned])
    assert not any(bool((index == copy).any()) for _, copy in moves)


@pytest.mark.parametrize("k", list(range(len(ref.SHAPES))) + ["translated"])
def test_both_directions_are_one_function(k):
    """A (point, triangle) pair has the same float32 distance whichever search evaluates it: the least distance of
    an image is the same number from both, bit for bit, and the point -> triangle minimum at the point a triangle
    chose, a minimum over all triangles of that very point, never exceeds what the triangle reports for the pair."""
    p, v, tri = ref.mesh(k)
    pd, vd, td = p.to(DEV), v.to(DEV), tri.to(DEV)
    by_point = points.nearest_triangles(pd, vd, td)[0]
    by_triangle, index, _ = points.triangle_nearest_points(pd, vd, td)
    assert bool((index >= 0).all())
    assert torch.equal(by_triangle.min(dim=1).values, by_point.min(dim=1).values)
    assert bool((torch.gather(by_point, 1, index.long()) <= by_triangle).all())


@pytest.mark.parametrize("k", [3, 4])   # without and with a split
def test_unusable_triangles_never_get_a_result(k):
    p, v, tri = ref.mesh(k)
    B, N, V, T = ref.SHAPES[k]
    assert (_native.nearest_point_of_triangle_plan(B, N, T)["splits"] > 1) == (k == 4)
    lengths = torch.tensor([N, N // 2, 1][:B])
    mixed = tri.clone()
    mixed[::2, 0] = -1
    mixed[1::4, 2] = V
    usable = ((mixed >= 0) & (mixed < V)).all(dim=1)
    pg, vg = p.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    out = points.triangle_nearest_points(pg, vg, mixed.to(DEV), lengths.to(DEV))
    _check(p, v, mixed, out, "unusable triangles %d" % k, lengths)
    index = out[1].cpu().long()
    assert bool((index[:, ~usable] == -1).all()) and bool((index[:, usable] >= 0).all())
    assert bool((index < lengths[:, None]).all())
    mean = points.mesh_point_distance(pg, vg, mixed.to(DEV), lengths.to(DEV))
    want_mean = out[0].detach().double().sum(1) / int(usable.sum())
    assert float((mean.detach().double() - want_mean).abs().max()) <= 1e-5 * float(want_mean.max())
    mean.sum().backward()
    _, wdv = mp.mean_gradients(p, v, mixed, index, out[2].cpu(), torch.ones(B))
    _grad_close(vg.grad, wdv, "unusable triangles %d mean dvertices" % k)
    # nothing usable at all
    none = torch.full_like(tri, V)
    none[::3] = -1
    pg, vg = p.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    sqdist, index, bary = points.triangle_nearest_points(pg, vg, none.to(DEV))
    mean = points.mesh_point_distance(pg, vg, none.to(DEV))
    assert bool((index == -1).all()) and bool((sqdist == 0).all()) and bool((bary == 0).all()) and bool((mean == 0).all())
    (sqdist.sum() + mean.sum()).backward()
    assert bool((pg.grad == 0).all()) and bool((vg.grad == 0).all())


@pytest.mark.parametrize("k", [3, 4])   # without and with a split
def test_non_finite_coordinates_keep_the_indices_in_range(k):
    p, v, tri = ref.mesh(k)
    B, N, V, T = ref.SHAPES[k]
    mixed = tri.clone()
    mixed[::5, 1] = V
    usable = ((mixed >= 0) & (mixed < V)).all(dim=1)
    clean = points.triangle_nearest_points(p.to(DEV), v.to(DEV), mixed.to(DEV))
    bad_p, bad_v = p.clone(), v.clone()
    bad_p[0, 5, 1] = float("nan")
    bad_p[1, 9, 0] = float("inf")
    bad_p[1, 10] = float("-inf")
    bad_v[0, 7, 2] = float("nan")
    bad_v[1, 11, 0] = float("-inf")
    pg, vg = bad_p.to(DEV).requires_grad_(True), bad_v.to(DEV).requires_grad_(True)
    sqdist, index, bary = points.triangle_nearest_points(pg, vg, mixed.to(DEV))
    host = index.cpu().long()
    assert bool((host >= -1).all()) and bool((host < N).all()) and bool((host[:, ~usable] == -1).all())
    assert not bool((host[0] == 5).any()) and not bool((host[1] == 9).any()) and not bool((host[1] == 10).any())
    assert not bool(torch.isnan(sqdist).any()) and not bool(torch.isnan(bary).any())
    assert bool(torch.isfinite(sqdist).all()) and bool((bary >= 0).all())
    for b, vertex, lost in ((0, 7, (5,)), (1, 11, (9, 10))):   # triangles that never met what was poisoned are unchanged
        same = usable & ~(mixed == vertex).any(dim=1)
        for j in lost:
            same &= clean[1][b].cpu() != j
        assert bool(same.any()) and bool((host[b][same] >= 0).all())
        assert torch.equal(sqdist[b][same.to(DEV)], clean[0][b][same.to(DEV)])
        assert torch.equal(index[b][same.to(DEV)], clean[1][b][same.to(DEV)])
    sqdist.sum().backward()                    # reads nothing out of range; the values may be non-finite
    mean = points.mesh_point_distance(pg, vg, mixed.to(DEV))
    mean.sum().backward()
    # a cloud of nothing but NaN: no result anywhere
    nothing = points.triangle_nearest_points(torch.full_like(p, float("nan")).to(DEV), v.to(DEV), tri.to(DEV))
    assert bool((nothing[1] == -1).all()) and bool((nothing[0] == 0).all()) and bool((nothing[2] == 0).all())
    torch.cuda.synchronize()


def test_lengths_and_poisoned_padding():
    p, v, tri, lengths = mp.case(("own", 6))            # lengths 700, 0, 333: three splits
    assert _native.nearest_point_of_triangle_plan(3, 700, 90)["splits"] == 3
    td, ld = tri.to(DEV), lengths.to(DEV)
    g = torch.Generator().manual_seed(5)
    upstream = torch.randn(3, 90, generator=g).to(DEV)
    runs = []
    for poison in (None, float("nan"), float("inf"), 3.0e38):
        cloud = p.clone()
        if poison is not None:
            for b in range(3):
                cloud[b, int(lengths[b]):] = poison
        pg, vg = cloud.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
        out = points.triangle_nearest_points(pg, vg, td, ld)
        out[0].backward(upstream)
        mean = points.mesh_point_distance(pg, vg, td, ld)
        mp_, mv_ = torch.autograd.grad(mean.sum(), (pg, vg))
        runs.append(tuple(t.detach() for t in out) + (pg.grad, vg.grad, mean.detach(), mp_, mv_))
    for other in runs[1:]:                     # the padding influences nothing, bit for bit
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    sqdist, index, bary, dp, dv, mean, mdp, mdv = runs[0]
    assert bool((index[1] == -1).all()) and bool((sqdist[1] == 0).all()) and bool((bary[1] == 0).all())
    assert float(mean[1]) == 0.0 and bool((dp[1] == 0).all()) and bool((dv[1] == 0).all())
    assert bool((mdp[1] == 0).all()) and bool((mdv[1] == 0).all())
    assert bool((dp[2, 333:] == 0).all()) and bool((mdp[2, 333:] == 0).all())
    # lengths beyond the cloud are clamped by the kernel, int64 lengths are taken
    over = points.triangle_nearest_points(p.to(DEV), v.to(DEV), td, torch.tensor([9999, 700, 2 ** 40], device=DEV))
    for a, b in zip(over, points.triangle_nearest_points(p.to(DEV), v.to(DEV), td)):
        assert torch.equal(a, b)


def test_input_forms():
    p, v, tri = ref.mesh(3)
    pd, vd, td = p.to(DEV), v.to(DEV), tri.to(DEV)
    whole = points.triangle_nearest_points(pd, vd, td)
    assert not whole[1].requires_grad and not whole[2].requires_grad
    # a non-contiguous view, and its gradient
    wide = torch.zeros(3, 65, 6, device=DEV)
    wide[..., 1::2] = pd
    leaf = wide.requires_grad_(True)
    out = points.triangle_nearest_points(leaf[..., 1::2], vd, td.t().contiguous().t())
    for a, b in zip(out, whole):
        assert torch.equal(a.detach(), b)
    assert not out[1].requires_grad and not out[2].requires_grad
    upstream = torch.ones_like(out[0])
    out[0].backward(upstream)
    wdp, _ = mp.gradients(p, v, tri, out[1].cpu(), out[2].cpu(), upstream.cpu())
    _grad_close(leaf.grad[..., 1::2], wdp, "non-contiguous dpoints")
    assert bool((leaf.grad[..., 0::2] == 0).all()) and vd.grad is None
    # every integer dtype of the triangles, on the host too
    for dtype in (torch.int64, torch.int32, torch.int16):
        for a, b in zip(points.triangle_nearest_points(pd, vd, tri.to(dtype)), whole):
            assert torch.equal(a, b)
    # no gradient wanted: no backward node
    assert whole[0].grad_fn is None and points.mesh_point_distance(pd, vd, td).grad_fn is None
    # without the batch axis, a 0-dim length
    one = points.triangle_nearest_points(pd[1], vd[1], td, lengths=torch.tensor(65, device=DEV))
    assert one[0].shape == (63,) and one[1].shape == (63,) and one[2].shape == (63, 3)
    for a, b in zip(one, whole):
        assert torch.equal(a, b[1])
    mean = points.mesh_point_distance(pd[1], vd[1], td)
    assert mean.dim() == 0 and abs(float(mean) - float(whole[0][1].double().mean())) <= 1e-5 * float(mean)
    both = points.point_mesh_face_distance(pd, vd, td)
    assert torch.equal(both, points.point_mesh_distance(pd, vd, td) + points.mesh_point_distance(pd, vd, td))
    assert points.point_mesh_face_distance(pd[1], vd[1], td).dim() == 0
    # float64 on the device takes the torch path
    sqdist, index, bary = points.triangle_nearest_points(pd.double(), vd.double(), td)
    want, _, _ = mp.cached_nearest(("ref", 3))
    assert sqdist.dtype == torch.float64 and sqdist.is_cuda and index.dtype == torch.int32
    assert float((sqdist.cpu() - want).abs().max()) <= 1e-12
    with pytest.raises(RuntimeError):
        points.triangle_nearest_points(pd, v, td)    # points and vertices on two devices
    with pytest.raises(RuntimeError):
        points.triangle_nearest_points(pd, vd, td, lengths=torch.tensor([1, 2, 3]))   # lengths on the host
    with pytest.raises(RuntimeError):
        points.mesh_point_distance(pd, vd.double(), td)
    with pytest.raises(ValueError):
        points.point_mesh_face_distance(pd, vd[:2], td)


def test_bitwise_reproducible_in_either_mode():
    p, v, tri, _ = mp.case(("own", 2))          # (1, 300, 60, 257): two splits, two workgroups of triangles
    g = torch.Generator().manual_seed(6)
    upstream = torch.randn(1, 257, generator=g).to(DEV)
    td = tri.to(DEV)

    def run():
        pg, vg = p.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
        sqdist, index, bary = points.triangle_nearest_points(pg, vg, td)
        sqdist.backward(upstream)
        mean = points.mesh_point_distance(pg, vg, td)
        mdp, mdv = torch.autograd.grad(mean.sum(), (pg, vg))
        return sqdist.detach(), index, bary, pg.grad, vg.grad, mean.detach(), mdp, mdv

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


def test_captured_step_with_the_face_distance_and_the_regulariser():
    vertices, triangles, _ = shapes.sphere(1.0, 6)
    B, V = 2, vertices.shape[0]
    tri = triangles.to(DEV)
    g = torch.Generator().manual_seed(9)
    v = (vertices[None] + 0.03 * torch.randn(B, V, 3, generator=g)).to(DEV).requires_grad_(True)
    scan = (torch.randn(B, 700, 3, generator=g) * torch.tensor([1.4, 0.8, 1.0])).to(DEV)
    lengths = torch.tensor([700, 450], device=DEV)
    reg.mesh_topology(tri, V)              # reads counts back: built before the capture

    def loss_of(m):
        return (points.point_mesh_face_distance(scan, m, tri, lengths) + reg.mesh_regularizer(m, tri, 0.3, 0.2, 0.1)).sum()

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
    # the mesh-to-point part of the replayed step is the restatement's
    only = v.detach().clone().requires_grad_(True)
    mean = points.mesh_point_distance(scan, only, tri, lengths)
    mean.sum().backward()
    host_v, host_scan, host_len = v.detach().cpu(), scan.cpu(), lengths.cpu()
    want, want_index, _ = mp.nearest(host_scan, host_v, triangles, host_len)
    want_mean = mp.mean_of(want, host_v, triangles)
    atol = mp.mean_atol(host_scan, host_v, triangles, want_index, mp.HIP_BOUND_UNITS)
    assert bool(((mean.detach().double().cpu() - want_mean).abs() <= 1e-5 * want_mean + atol).all())
    _, index, bary = points.triangle_nearest_points(scan, v.detach(), tri, lengths)
    _, wdv = mp.mean_gradients(host_scan, host_v, triangles, index.cpu(), bary.cpu(), torch.ones(B))
    _grad_close(only.grad, wdv, "captured mesh-to-point dvertices")
