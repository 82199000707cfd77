"""mesh_renderer.points.winding_number / inside_mesh / signed_distance on the MI355X (the k_wn_* kernels of
csrc/nearest.hip) against the float64 restatement (tests/winding_reference.py).

Forward bound, per query and with no query exempt:  E_i = 2^-24 sum_f (16 * 2 M_f / r_f + 4 |Omega_f|) / (4 pi) +
T 2^-41, M = |a||b||c|, r = hypot(num, den), Omega = 2 atan2(num, den) in float64.  The constant 16: an error (dn, dd)
in (num, den) moves atan2 by at most hypot(dn, dd) / r, and each of num and den is about a dozen float32 roundings of
magnitude <= M.  With 1 in its place the float32 torch evaluation on the CPU reaches 2.9 E; with 16 it stays at or
below 0.21 E, which leaves the kernels (their own fused multiply-adds, a 1-ulp square root, another atan2) a factor of
about 5.  WORST MEASURED err/E of the kernels on the MI355X (2026-10-20): 0.180, on the single-triangle soup
(2, 300, 3, 1); per case 0 / 0.180 / 0.070 / 0.008 / 0.031 / 0.070 / 0.096 / 0.030 on the soups 0, 2, 3, 5, 6, 7, 8 and
"translated", 0.086 on the cube, 0.004 and 0.002 on the sphere plain and translated, 0.024 on the batch of 64 whose
splits hold two tiles each.  The share of queries with E_i <= 1e-3 is 1.0 everywhere except 0.925 on (1, 40, 900, 5000).

The bit-for-bit tests are what the 64-bit fixed-point sum (csrc/wn_fixed.h) promises: the same w whatever the order
of the triangles, the split of their range, the batch an image sits in."""
import pytest
import torch

import point_mesh_reference as pm
import winding_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
points = mesh_renderer.points


def _plan(p, tri):
    return _native.winding_number_plan(p.shape[0], p.shape[1], tri.shape[0])


def _wn(p, v, tri, lengths=None):
    return points.winding_number(p.to(DEV), v.to(DEV), tri.to(DEV), None if lengths is None else lengths.to(DEV))


def test_the_cases_reach_both_routes_and_both_kernels():
    plans = [_plan(*ref.case(name)[::2]) for name in ref.NAMES]
    assert any(pl["splits"] > 1 for pl in plans) and any(pl["splits"] == 1 for pl in plans)
    for lanes in (1, 2):
        assert any(pl["splits"] > 1 and pl["queries_per_lane"] == lanes for pl in plans)
        assert any(pl["splits"] == 1 and pl["queries_per_lane"] == lanes for pl in plans)


@pytest.mark.parametrize("name", ref.NAMES)
def test_winding_number_matches_the_restatement(name):
    p, v, tri = ref.case(name)
    want, bound = ref.truth(name)
    w = points.winding_number(p.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True), tri.to(DEV))
    assert w.dtype == torch.float32 and w.shape == p.shape[:2] and w.is_cuda
    assert not w.requires_grad and w.grad_fn is None
    ref.check(w, want, bound, "%s %s" % (name, _plan(p, tri)))
    one = points.winding_number(p[0].to(DEV), v[0].to(DEV), tri.to(torch.int32).to(DEV))   # without the batch axis
    assert one.shape == p.shape[1:2] and torch.equal(one, w[0])


@pytest.mark.parametrize("name", ["soup_5", "soup_7", "soup_8", "sphere"])
def test_a_permutation_of_the_triangles_changes_nothing(name):
    p, v, tri = ref.case(name)
    perm = torch.randperm(tri.shape[0], generator=torch.Generator().manual_seed(11))
    assert torch.equal(_wn(p, v, tri[perm]), _wn(p, v, tri))


def test_a_batch_equals_its_single_image_calls():
    for name in ("soup_3", "soup_7", "cube"):
        p, v, tri = ref.case(name)
        whole = _wn(p, v, tri)
        for b in range(p.shape[0]):
            assert torch.equal(_wn(p[b:b + 1], v[b:b + 1], tri)[0], whole[b]), (name, b)
    # 256 workgroups of two queries a lane leave 3 splits of two tiles each; one image alone gets 6 splits of one
    g = torch.Generator().manual_seed(12)
    p, v = torch.rand(64, 2048, 3, generator=g) * 2 - 1, torch.rand(64, 90, 3, generator=g) * 2 - 1
    tri = torch.randint(0, 90, (700, 3), generator=g)
    many, alone = _plan(p, tri), _plan(p[:1], tri)
    assert 1 < many["splits"] < alone["splits"] and many["queries_per_lane"] == 2
    whole = _wn(p, v, tri)
    for b in (0, 37, 63):
        assert torch.equal(_wn(p[b:b + 1], v[b:b + 1], tri)[0], whole[b])
    want, bound = ref.winding(p[63:, :300], v[63:], tri)
    ref.check(whole[63:, :300], want, bound, "two tiles a split")


def test_lengths_equal_the_truncated_call():
    p, v, tri = ref.case("soup_7")
    counts = [300, 0]
    out = _wn(p, v, tri, torch.tensor(counts))
    for b, n in enumerate(counts):
        assert bool((out[b, n:] == 0).all())
        if n:
            assert torch.equal(out[b, :n], _wn(p[b:b + 1, :n], v[b:b + 1], tri)[0])
    over = _wn(p, v, tri, torch.tensor([9999, 2 ** 40]))
    assert torch.equal(over, _wn(p, v, tri))


@pytest.mark.parametrize("name", ["soup_3", "soup_7"])
def test_skipped_triangles_change_nothing(name):
    p, v, tri = ref.case(name)
    V = v.shape[1]
    junk = torch.tensor([[0, 1, V], [-1, 2, 3], [4, 4, 5], [6, 7, 6], [8, 8, 8], [2 ** 40, 0, 1]])
    base = _wn(p, v, tri)
    assert torch.equal(_wn(p, v, torch.cat([junk, tri[:40], junk, tri[40:], junk])), base)
    assert bool((_wn(p, v, junk) == 0).all())   # nothing but skipped triangles


def test_non_finite_input():
    p, v, tri = ref.case("soup_7")   # two queries a lane, two splits
    base = _wn(p, v, tri)
    bad = p.clone()
    bad[0, 3, 1] = float("nan")
    bad[1, 400, 0] = float("inf")
    bad[1, 512, 2] = float("-inf")
    w = _wn(bad, v, tri)
    hit = torch.zeros(base.shape, dtype=torch.bool, device=DEV)
    hit[0, 3] = hit[1, 400] = hit[1, 512] = True
    assert bool(torch.isnan(w[hit]).all()) and torch.equal(w[~hit], base[~hit])
    bad_v = v.clone()
    bad_v[1, int(tri[128, 0])] = float("nan")   # a vertex of the LAST split's only triangle
    w = _wn(p, bad_v, tri, torch.tensor([513, 100]))
    assert torch.equal(w[0], base[0]) and bool(torch.isnan(w[1, :100]).all()) and bool((w[1, 100:] == 0).all())
    assert not bool(points.inside_mesh(p.to(DEV), bad_v.to(DEV), tri.to(DEV))[1].any())
    # without a split
    p, v, tri = ref.case("soup_8")
    base = _wn(p, v, tri)
    bad = p.clone()
    bad[0, 300] = float("nan")
    w = _wn(bad, v, tri)
    assert bool(torch.isnan(w[0, 300])) and torch.equal(w[0, :300], base[0, :300]) and torch.equal(w[0, 301:], base[0, 301:])


def test_cube_inside_and_signed_distance():
    p, v, tri = ref.case("cube")
    exact = ref.box_signed_distance(p)
    clear = exact.abs() >= 0.01
    pd, vd, td = p.to(DEV), v.to(DEV), tri.to(DEV)
    inside = points.inside_mesh(pd, vd, td)
    assert inside.dtype == torch.bool and inside.shape == p.shape[:2] and inside.is_cuda
    assert torch.equal(inside.cpu()[clear], (p.abs().max(-1).values < 0.5)[clear])
    assert bool(inside.any()) and not bool(inside.all())
    assert not bool(points.inside_mesh(pd, vd, td, torch.tensor([300, 7], device=DEV))[1, 7:].any())

    pg, vg = pd.clone().requires_grad_(True), vd.clone().requires_grad_(True)
    sd = points.signed_distance(pg, vg, td)
    sqdist, face, bary = points.nearest_triangles(pd, vd, td)
    assert sd.dtype == torch.float32 and sd.shape == p.shape[:2] and sd.grad_fn is not None
    assert torch.equal(sd.detach().abs(), sqdist.sqrt())
    assert bool(((sd.detach().cpu() < 0) == (exact < 0))[clear].all())
    assert torch.equal(sd.detach() < 0, inside & (sqdist > 0))
    # d(s sqrt(q)) = s / (2 d) dq: the restatement's gradient of sum_i u_i |p_i - c_i|^2 at the returned face and
    # barycentrics with u = g s / (2 d)
    g = torch.randn(sd.shape, generator=torch.Generator().manual_seed(13))
    sd.backward(g.to(DEV))
    d = sqdist.sqrt().double().cpu()
    s = torch.where(inside.cpu(), -1.0, 1.0).double()
    assert bool((d > 0).all())
    wdp, wdv = pm.gradients(p, v, tri, face.cpu(), bary.cpu(), g.double() * s / (2.0 * d))
    for got, want, what in ((pg.grad, wdp, "dpoints"), (vg.grad, wdv, "dvertices")):
        scale = float(want.abs().max())
        err = float((got.double().cpu() - want).abs().max())
        print("signed_distance %s: gradient max err %.3g of scale %.3g" % (what, err, scale))
        assert err <= 1e-4 * scale
    # a query placed on a vertex of the cube: distance 0, gradient 0, not NaN
    on = vd[:1, 5:6].clone().requires_grad_(True)
    alone = vd[:1].clone().requires_grad_(True)
    zero = points.signed_distance(on, alone, td)
    zero.sum().backward()
    assert float(zero.detach()) == 0.0 and bool((on.grad == 0).all()) and bool((alone.grad == 0).all())


def test_open_sphere_centre():
    p, v, tri = ref.case("sphere")
    want, bound = ref.truth("sphere")
    assert abs(float(want[0, 0]) - 0.96) < 1e-3
    w = _wn(p[:, :1], v, tri)
    err = abs(float(w[0, 0]) - float(want[0, 0]))
    print("centre of the open sphere: w %.7f, float64 %.7f, err/E %.3f" % (float(w[0, 0]), float(want[0, 0]), err / float(bound[0, 0])))
    assert err <= float(bound[0, 0])
    assert bool(points.inside_mesh(p[0, :1].to(DEV), v[0].to(DEV), tri.to(DEV))[0])


@pytest.mark.parametrize("name", ["soup_7", "soup_8"])
def test_graph_capture_replays_the_eager_result(name):
    p, v, tri = ref.case(name)
    pd, vd, td = p.to(DEV), v.to(DEV), tri.to(DEV)
    eager = points.winding_number(pd, vd, td)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        points.winding_number(pd, vd, td)   # warm up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = points.winding_number(pd, vd, td)
    captured.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
    pd.copy_(pd.flip(1))   # new inputs in place: the replay follows them
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager.flip(1))
