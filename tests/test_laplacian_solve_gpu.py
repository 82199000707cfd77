"""mesh_renderer.preconditioning on the MI355X (csrc/mesh_solve.hip) against the float64 truth of
tests/laplacian_solve_reference.py.

Accuracy, per (image, channel):  |x_dev - x64| / |b|  <=  max(tol, 4 x cg32's error on the same case).  cg32 is the
float32 restatement of the algorithm; a device recurrence that differs from it in its summation orders alone gets
four times its error, and nothing is compared with the code under test.  iterations < max_iterations is asserted
everywhere: the restatement needs at most 73 on these inputs, and a solver that never converges must not pass on
the accuracy of its last iterate.  Every case runs on the planned route and with the stepped route forced.  On the
MI355X the device's error is at most 0.26 of the bound over all cases, the strips included."""
import numpy as np
import pytest
import torch

import laplacian_solve_reference as lref
from pytorch_mesh_renderer_amd import _native, mesh_renderer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
pre = mesh_renderer.preconditioning
RESIDENT, STEPS = _native.LAPLACIAN_ROUTE_RESIDENT, _native.LAPLACIAN_ROUTE_STEPS
ROUTES = (None, STEPS)
# every V after which laplacian_solve_plan(V, 3) changes, and V + 1, and around one wavefront: what _launch_sizes()
# finds by bisection (test_the_shapes_cover_every_launch_path holds the two equal)
LAUNCH_SIZES = [1, 2, 3, 63, 64, 65, 128, 129, 1024, 1025, 3072, 3073, 262144, 262145]
SMALL = 1 + 2.0 ** -10     # the "(1 + small)" of a rounding bound: second-order terms


_topologies = {}


def _topology(kind):
    if kind not in _topologies:
        _, triangles = lref.tensors(kind, DEV)
        _topologies[kind] = _native.mesh_topology(triangles, lref.mesh(kind)[0].shape[0])
    return _topologies[kind]


def _solve(kind, lam, b, route=None, **settings):
    """b: numpy or device tensor [B,V,C] -> (x, iterations, residual) on the device."""
    if not torch.is_tensor(b):
        b = torch.from_numpy(np.ascontiguousarray(b)).to(DEV)
    return _native.laplacian_solve(b, _topology(kind), lam, route=route, **settings)


def _same(a, b):
    return all(p.dtype == q.dtype and p.cpu().numpy().tobytes() == q.cpu().numpy().tobytes() for p, q in zip(a, b))


def _shape_of(V):
    p = _native.laplacian_solve_plan(V, 3)
    return (p["route"], p["workgroup_size"], p["vertices_per_lane"])


def _changes(lo, hi):
    """Every V in [lo, hi) whose launch shape differs from that of V + 1, by bisection."""
    if _shape_of(lo) == _shape_of(hi):
        return []
    if hi == lo + 1:
        return [lo]
    mid = (lo + hi) // 2
    return _changes(lo, mid) + _changes(mid, hi)


def _boundaries():
    marks = sorted({1} | {2 ** e for e in range(1, 20)} | {3 * 2 ** e for e in range(18)})
    return [n for lo, hi in zip(marks[:-1], marks[1:]) for n in _changes(lo, hi)]


def _launch_sizes():
    return sorted({1, 2, 3, 63, 64, 65} | {V for n in _boundaries() for V in (n, n + 1)})


@pytest.mark.parametrize("lam", lref.LAMBDAS)
@pytest.mark.parametrize("kind", lref.MESHES)
def test_accuracy_against_the_truth(kind, lam):
    for C in lref.CHANNELS:
        case = lref.case(kind, lam, C)
        limit = lref.bound(case["cg32_error"])
        for route in ROUTES:
            x, iterations, residual = _solve(kind, lam, case["b"], route)
            assert x.dtype == torch.float32 and x.shape == case["b"].shape
            assert iterations.dtype == torch.int32 and residual.dtype == torch.float32
            assert iterations.shape == residual.shape == (3, C)
            error = lref.relative_error(x.cpu().numpy(), case["x64"], case["b"])
            print("%s lam %g C %d route %s: error / bound %.2f, iterations %d (cg32 %d)" % (
                kind, lam, C, route, (error / limit).max(), int(iterations.max()), case["cg32_iterations"].max()))
            assert int(iterations.max()) < lref.MAX_ITERATIONS, (C, route, iterations.tolist())
            assert bool((residual <= lref.TOL).all()), (C, route, residual.tolist())
            assert (error <= limit).all(), (C, route, error.tolist(), limit.tolist())
    public = pre.from_differential(torch.from_numpy(case["b"]).to(DEV), lref.tensors(kind, DEV)[1], lam)
    assert _same([public], [_solve(kind, lam, case["b"])[0]])


def test_the_shapes_cover_every_launch_path():
    bounds, sizes = _boundaries(), _launch_sizes()
    assert sizes == LAUNCH_SIZES
    shapes_tested = {_shape_of(V) for V in sizes}
    last_resident = max(n for n in bounds if _shape_of(n)[0] == 1)
    assert _shape_of(last_resident + 1)[0] == 2 and {last_resident, last_resident + 1} <= set(sizes)
    assert last_resident * 16 <= 160 * 1024                                   # p of four channels fits a CU's LDS
    assert _native.laplacian_solve_plan(1 << 22, 3)["route"] == 2             # and it stays with the stepped route
    assert any(s[0] == 1 and s[1] == 64 for s in shapes_tested)               # the one-wavefront shape
    every = {_shape_of(V) for n in bounds + [1] for V in (n, n + 1)}
    assert every <= shapes_tested
    assert {s[1] for s in every if s[0] == 1} == {s[1] for s in shapes_tested if s[0] == 1} and len(every) >= 4
    assert any(s[0] == 2 and s[2] > 1 for s in shapes_tested)                 # more than one vertex a lane, stepped
    for C in (1, 2, 4):                                                       # the plan's V boundaries hold for every C
        for V in sizes:
            p = _native.laplacian_solve_plan(V, C)
            assert (p["route"], p["workgroup_size"], p["vertices_per_lane"]) == _shape_of(V)


@pytest.mark.parametrize("V", LAUNCH_SIZES)
def test_every_boundary_of_the_plan(V):
    """strip(V) at every V after which the route, the workgroup size or the vertices per lane change, at V + 1, and
    around one wavefront; the right-hand side is the vertices.  lam = 19 (the stiffness the fits use) up to 10000
    vertices, lam = 1 above, where the float64 truth is itself a CG."""
    kind, lam = "strip%d" % V, (19.0 if V <= 10000 else 1.0)
    b = lref.mesh(kind)[0][None]
    x64 = lref.truth(kind, lam, b)
    x32, cg32_iterations, _ = lref.cg32(lref.system64(kind, lam), b[0])
    limit = lref.bound(lref.relative_error(x32[None], x64, b))
    routes = (None, STEPS) if _shape_of(V)[0] == 1 else (None,)
    for route in routes:
        x, iterations, residual = _solve(kind, lam, b, route)
        error = lref.relative_error(x.cpu().numpy(), x64, b)
        print("strip(%d) %s route %s: error / bound %.2f, iterations %d (cg32 %d)" % (
            V, _shape_of(V), route, (error / limit).max(), int(iterations.max()), cg32_iterations.max()))
        assert int(iterations.max()) < lref.MAX_ITERATIONS and int(iterations.min()) >= 1
        assert (error <= limit).all(), (route, error.tolist(), limit.tolist())
    if _shape_of(V)[0] == 2:
        with pytest.raises(ValueError):
            _solve(kind, lam, b, RESIDENT)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", ["sphere8", "sphere25"])
def test_bit_for_bit_properties(kind, route):
    lam = 19.0
    b = torch.from_numpy(lref.batch(kind, 3)).to(DEV)
    whole = _solve(kind, lam, b, route)
    assert _same(whole, _solve(kind, lam, b, route))                                       # two runs
    assert _same(whole, _solve(kind, lam, b, route, x0=torch.zeros_like(b)))               # x0 = 0 is no x0
    assert _same(whole, _solve(kind, lam, b, route, check_every=7))                        # stopping early changes nothing
    per_image = whole[1].max(dim=1).values.tolist()
    assert len(set(per_image)) > 1, per_image                                              # they freeze at different iterations
    for k in range(3):                                                                     # the batch equals its singles
        one = _solve(kind, lam, b[k:k + 1].contiguous(), route)
        assert _same([t[0] for t in one], [t[k] for t in whole]), k
    lo, hi = int(whole[1].min()), int(whole[1].max())
    M = (lo + hi + 1) // 2
    short = _solve(kind, lam, b, route, max_iterations=M)
    longer = _solve(kind, lam, b, route, max_iterations=M + 64)
    frozen = (short[1] < M).cpu()
    assert bool(frozen.any()) and not bool(frozen.all())
    assert _same([short[0].cpu().transpose(1, 2)[frozen], short[1].cpu()[frozen], short[2].cpu()[frozen]],
                 [longer[0].cpu().transpose(1, 2)[frozen], longer[1].cpu()[frozen], longer[2].cpu()[frozen]])
    assert bool((short[1].cpu()[~frozen] == M).all())
    if M + 64 > hi:                                                                        # past the last freeze
        assert _same(longer, whole)
    # a NaN image leaves the other two images' bits unchanged, and its clean channels too
    bad = b.clone()
    bad[1, 5, 0] = float("nan")
    got = _solve(kind, lam, bad, route)
    assert bool(torch.isnan(got[0][1, :, 0]).all()) and int(got[1][1, 0]) == 0 and bool(torch.isnan(got[2][1, 0]))
    assert _same([t[k] for t in got for k in (0, 2)], [t[k] for t in whole for k in (0, 2)])
    assert _same([got[0][1, :, 1:], got[1][1, 1:], got[2][1, 1:]], [whole[0][1, :, 1:], whole[1][1, 1:], whole[2][1, 1:]])


@pytest.mark.parametrize("route", ROUTES)
def test_freeze_rules_on_the_device(route):
    kind, lam = "sphere8", 19.0
    b = torch.from_numpy(lref.batch(kind, 2)).to(DEV)
    zero = b.clone()
    zero[1] = 0
    x, iterations, residual = _solve(kind, lam, zero, route)
    assert bool((x[1] == 0).all()) and iterations[1].tolist() == [0, 0] and residual[1].tolist() == [0.0, 0.0]
    x, iterations, residual = _solve(kind, lam, b, route, max_iterations=0)
    assert bool((x == 0).all()) and bool((iterations == 0).all()) and bool((residual == 1).all())
    start = torch.from_numpy(np.random.default_rng(3).standard_normal(b.shape).astype(np.float32)).to(DEV)
    x, iterations, _ = _solve(kind, lam, b, route, max_iterations=0, x0=start)
    assert torch.equal(x, start) and bool((iterations == 0).all())
    # tol = 0 runs every system until r = 0, breakdown or the last iteration: finite, and as accurate as float32 gets
    x, iterations, residual = _solve(kind, lam, b, route, tol=0.0, max_iterations=600)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(residual).all()) and int(iterations.max()) <= 600
    x64 = lref.truth(kind, lam, b.cpu().numpy())
    assert lref.relative_error(x.cpu().numpy(), x64, b.cpu().numpy()).max() <= 1e-5
    # a warm start from the solution has only its own rounding left to remove
    cold = _solve(kind, lam, b, route)
    warm = _solve(kind, lam, b, route, x0=cold[0])
    assert bool((warm[1] < cold[1]).all())
    error = lref.relative_error(warm[0].cpu().numpy(), x64, b.cpu().numpy())
    assert (error <= lref.bound(lref.case(kind, lam, 2)["cg32_error"])).all()


@pytest.mark.parametrize("kind", ["sphere25", "fan300", "strays", "strip3073"])
def test_to_differential_against_float64(kind):
    """|err_i| <= (deg_i + 3) 2^-24 ((1 + lam deg_i) |x_i| + lam sum |x_j|) (1 + small): the rounding of a sum of
    deg_i + 3 float32 terms, the diagonal and lam among them."""
    vertices, triangles = lref.tensors(kind, DEV)
    V = vertices.shape[0]
    for lam in (0.0, 0.37, 19.0):
        system = lref.System64(lref.mesh(kind)[1], V, float(np.float32(lam)))
        for C in lref.CHANNELS:
            x = np.random.default_rng(V + C).standard_normal((2, V, C)).astype(np.float32)
            got = pre.to_differential(torch.from_numpy(x).to(DEV), triangles, lam)
            assert got.dtype == torch.float32 and got.shape == x.shape
            for k in range(2):
                error = np.abs(got[k].cpu().numpy().astype(np.float64) - system @ x[k])
                limit = (system.degree[:, None] + 3) * 2.0 ** -24 * system.absolute(x[k]) * SMALL
                assert (error <= limit).all(), (lam, C, float((error / np.maximum(limit, 1e-300)).max()))
            if lam == 0.0:
                assert np.array_equal(got.cpu().numpy(), x)
        single = pre.to_differential(torch.from_numpy(x[1]).to(DEV), triangles, lam)
        assert torch.equal(single, got[1])


def test_autograd_on_the_device():
    kind, lam = "sphere25", 19.0
    _, triangles = lref.tensors(kind, DEV)
    rng = np.random.default_rng(11)
    u_host, w_host = (rng.standard_normal((2, 627, 3)).astype(np.float32) for _ in range(2))
    w = torch.from_numpy(w_host).to(DEV)
    # from_differential: d sum(w . A^-1 u) / du = A^-1 w, within the accuracy bound of a solve of w
    u = torch.from_numpy(u_host).to(DEV).requires_grad_(True)
    x, iterations, residual = pre.from_differential(u, triangles, lam, return_info=True)
    assert x.requires_grad and not iterations.requires_grad and not residual.requires_grad
    (w * x).sum().backward()
    x64 = lref.truth(kind, lam, w_host)
    x32 = np.stack([lref.cg32(lref.system64(kind, lam), w_host[k])[0] for k in range(2)])
    limit = lref.bound(lref.relative_error(x32, x64, w_host))
    error = lref.relative_error(u.grad.cpu().numpy(), x64, w_host)
    assert (error <= limit).all(), (error.tolist(), limit.tolist())
    assert torch.equal(u.grad, pre.from_differential(w, triangles, lam))                  # the same solve, bit for bit
    # x0 takes part in the forward and receives nothing
    start = x.detach().clone().requires_grad_(True)
    pre.from_differential(u, triangles, lam, x0=start).sum().backward()
    assert start.grad is None
    # to_differential: d sum(w . A x) / dx = A w
    v = torch.from_numpy(u_host).to(DEV).requires_grad_(True)
    (w * pre.to_differential(v, triangles, lam)).sum().backward()
    assert torch.equal(v.grad, pre.to_differential(w, triangles, lam))
    system = lref.system64(kind, lam)
    for k in range(2):
        error = np.abs(v.grad[k].cpu().numpy().astype(np.float64) - system @ w_host[k])
        assert (error <= (system.degree[:, None] + 3) * 2.0 ** -24 * system.absolute(w_host[k]) * SMALL).all()
    # the round trip
    back = pre.from_differential(pre.to_differential(w, triangles, lam), triangles, lam)
    assert float((back - w).norm() / w.norm()) < 1e-4


@pytest.mark.parametrize("route", ROUTES)
def test_captured_solve_replays_to_the_eager_result(route):
    kind, lam = "sphere25", 19.0
    topology = _topology(kind)
    first = torch.from_numpy(lref.batch(kind, 3)).to(DEV)
    second = first.flip(0).contiguous() * 0.5
    static = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _native.laplacian_solve(static, topology, lam, route=route)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: the launches are a linear chain
        captured = _native.laplacian_solve(static, topology, lam, route=route)
    static.copy_(second)
    graph.replay()
    assert _same(captured, _native.laplacian_solve(second, topology, lam, route=route))
    assert not torch.equal(captured[0], _native.laplacian_solve(first, topology, lam, route=route)[0])


def test_captured_public_call_and_check_every_under_capture():
    kind, lam = "sphere8", 19.0
    _, triangles = lref.tensors(kind, DEV)
    topology = _topology(kind)
    first = torch.from_numpy(lref.batch(kind, 3)).to(DEV)
    second = first.flip(0).contiguous()
    static = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pre.from_differential(static, triangles, lam)   # (builds and caches the topology: that reads counts back)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x = pre.from_differential(static, triangles, lam, check_every=0)
        for call in (lambda: pre.from_differential(static, triangles, lam, check_every=4),
                     lambda: _native.laplacian_solve(static, topology, lam, check_every=4)):
            with pytest.raises(RuntimeError, match="capture"):
                call()
    static.copy_(second)
    graph.replay()
    assert torch.equal(x, pre.from_differential(second, triangles, lam))


def test_input_forms():
    kind, lam = "sphere8", 19.0
    vertices, triangles = lref.tensors(kind, DEV)
    b = torch.from_numpy(lref.batch(kind, 3)).to(DEV)
    wide = torch.zeros(3, 66, 6, device=DEV)
    wide[..., 1::2] = b
    view = wide[..., 1::2]
    assert not view.is_contiguous()
    plain = pre.from_differential(b, triangles, lam, return_info=True)
    assert _same(plain, pre.from_differential(view, triangles.long(), lam, return_info=True))
    one = pre.from_differential(b[1], triangles, lam, x0=torch.zeros_like(b[1]), return_info=True)
    assert one[0].shape == (66, 3) and one[1].shape == one[2].shape == (3,)
    assert _same(one, [t[1] for t in plain])
    assert torch.equal(pre.to_differential(view, triangles, lam), pre.to_differential(b, triangles, lam))
    # other dtypes take the torch route on the device
    x64 = pre.from_differential(b.double(), triangles, lam, tol=1e-10)
    assert x64.dtype == torch.float64 and x64.is_cuda
    assert float((x64 - plain[0].double()).norm() / x64.norm()) < 1e-5
    with pytest.raises(ValueError):
        _native.laplacian_solve(b, _native.mesh_topology(triangles, 67), lam)
    with pytest.raises(ValueError):
        pre.from_differential(b, triangles, lam, x0=torch.zeros(3, 66, 3))             # x0 on the host
