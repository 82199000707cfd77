"""Mesh regularisers on the MI355X against their float64 restatement (tests/mesh_regularizer_reference.py).

Budgets: values within 1e-5 relative, gradients within 1e-4 of the largest magnitude of the expected gradient
tensor (as test_sh_lighting_gpu.py).  A plain float32 torch evaluation of the same formulas on these meshes stays
within 1.5e-7 / 4e-6 of float64, so the budgets leave room for another summation order and nothing more."""
import importlib.util
import itertools
import os

import pytest
import torch

import mesh_regularizer_reference as ref
from conftest import ROOT
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
reg = mesh_renderer.regularizers

SUBSETS = [s for s in itertools.product((False, True), repeat=3) if any(s)]   # each alone, every pair, all three
_cache = {}


def _case(name):
    """-> (vertices [B,V,3] f32 host, triangles host, loop-built topology, dterms [B,3] f64), built once."""
    if name not in _cache:
        if name == "sphere6":
            vertices, triangles = ref.perturbed_sphere(6, 3, seed=1)
        elif name == "sphere12":
            vertices, triangles = ref.perturbed_sphere(12, 2, seed=2)
        elif name == "sphere20":
            vertices, triangles = ref.perturbed_sphere(20, 3, seed=3)
        elif name == "fan":
            v, triangles = ref.fan(70)
            vertices = torch.stack([v, v * torch.tensor([1.0, 0.8, 1.5])])
        elif name == "odd":
            v, triangles = ref.odd_mesh()
            vertices = torch.stack([v, v * torch.tensor([2.0, 1.0, 0.5]) + 0.25])   # the degeneracies stay exact
        g = torch.Generator().manual_seed(len(name))
        dterms = torch.randn(vertices.shape[0], 3, generator=g, dtype=torch.float64)
        _cache[name] = (vertices, triangles, ref.topology(triangles, vertices.shape[1]), dterms)
    return _cache[name]


def _check(got, got_grad, want, want_grad, what):
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_grad).all()), what
    err = (got.double().cpu() - want).abs()
    print("%s: values max rel err %.3g" % (what, float((err / want.abs().clamp(min=1e-30)).max())))
    assert bool((err <= 1e-5 * want.abs()).all()), "%s: values %s, expected %s" % (what, got.tolist(), want.tolist())
    scale = float(want_grad.abs().max())
    gerr = float((got_grad.double().cpu() - want_grad).abs().max())
    print("%s: gradient max err %.3g of scale %.3g" % (what, gerr, scale))
    assert gerr <= 1e-4 * scale, "%s: gradient error %.3g > 1e-4 * %.3g" % (what, gerr, scale)


def _run(vertices, triangles, dterms, **kwargs):
    leaf = vertices.to(DEV).requires_grad_(True)
    got = reg.mesh_terms(leaf, triangles, **kwargs)
    assert got.shape == (vertices.shape[0], 3) and got.dtype == torch.float32 and got.is_cuda
    got.backward(dterms.float().to(DEV))
    return got.detach(), leaf.grad


@pytest.mark.parametrize("target", [None, 0.35])
@pytest.mark.parametrize("subset", SUBSETS)
def test_sphere_matches_the_restatement(subset, target):
    vertices, triangles, topo, dterms = _case("sphere6")
    kwargs = dict(laplacian=subset[0], edge=subset[1], normal=subset[2], target_length=target)
    want, want_grad = ref.gradients(vertices, topo, dterms, **kwargs)
    got, grad = _run(vertices, triangles.to(DEV), dterms, **kwargs)
    _check(got, grad, want, want_grad, "sphere K=6 %s" % (kwargs,))
    for k, on in enumerate(subset):
        if not on:
            assert bool((got[:, k] == 0).all())


def test_sphere_input_forms():
    vertices, triangles, topo, dterms = _case("sphere6")
    want, want_grad = ref.gradients(vertices, topo, dterms)
    tri = triangles.to(DEV)
    # int64 triangles
    got, grad = _run(vertices, tri.long(), dterms)
    _check(got, grad, want, want_grad, "int64 triangles")
    # a non-contiguous view
    wide = torch.zeros(vertices.shape[0], vertices.shape[1], 6, device=DEV)
    wide[..., 1::2] = vertices.to(DEV)
    leaf = wide.requires_grad_(True)
    view = leaf[..., 1::2]
    assert not view.is_contiguous()
    out = reg.mesh_terms(view, tri)
    out.backward(dterms.float().to(DEV))
    _check(out.detach(), leaf.grad[..., 1::2], want, want_grad, "non-contiguous vertices")
    assert bool((leaf.grad[..., 0::2] == 0).all())
    # [V,3]: one image; the single-term functions return 0-dim tensors
    one = vertices[1].to(DEV).requires_grad_(True)
    out = reg.mesh_terms(one, tri)
    assert out.shape == (1, 3)
    out.backward(dterms[1:2].float().to(DEV))
    w1, g1 = ref.gradients(vertices[1:2], topo, dterms[1:2])
    _check(out.detach(), one.grad[None], w1, g1, "[V,3] vertices")
    for k, value in enumerate((reg.laplacian_smoothing(one, tri), reg.edge_length(one, tri),
                               reg.normal_consistency(one, tri))):
        assert value.dim() == 0 and abs(float(value.detach()) - float(w1[0, k])) <= 1e-5 * float(w1[0, k])
    total = reg.mesh_regularizer(vertices.to(DEV), tri, laplacian=0.5, edge=0.25, normal=2.0)
    want_total = (want * torch.tensor([0.5, 0.25, 2.0], dtype=torch.float64)).sum(1)
    assert total.shape == (3,) and float((total.double().cpu() - want_total).abs().max()) <= 1e-5 * float(want_total.max())
    # requires_grad=False: no backward node
    assert reg.mesh_terms(vertices.to(DEV), tri).grad_fn is None
    assert reg.mesh_regularizer(vertices.to(DEV), tri, laplacian=1.0).grad_fn is None
    for bad in (tri.float(), tri.bool()):
        with pytest.raises(RuntimeError, match="triangles must hold integer vertex indices"):
            reg.mesh_terms(vertices.to(DEV), bad)


@pytest.mark.parametrize("target", [None, 0.5])
def test_odd_mesh(target):
    vertices, triangles, topo, dterms = _case("odd")
    for subset in SUBSETS:
        kwargs = dict(laplacian=subset[0], edge=subset[1], normal=subset[2], target_length=target)
        want, want_grad = ref.gradients(vertices, topo, dterms, **kwargs)
        got, grad = _run(vertices, triangles.to(DEV), dterms, **kwargs)
        _check(got, grad, want, want_grad, "odd mesh %s" % (kwargs,))
        # the isolated vertex: exactly zero gradient from every term
        assert bool((grad[:, 9] == 0).all())
    # vertex 8 is in one flap only, as the far corner of a zero-area triangle: exactly zero gradient
    only_nc = dict(laplacian=False, edge=False, normal=True)
    _, want_grad = ref.gradients(vertices, topo, dterms, **only_nc)
    _, grad = _run(vertices, triangles.to(DEV), dterms, **only_nc)
    assert bool((want_grad[:, 8] == 0).all()) and bool((grad[:, 8] == 0).all())
    # a triangle collapsed to a point: delta = 0 and three zero-length edges, exactly zero gradients, no NaN
    point = torch.full((2, 3, 3), 0.75)
    tri = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=DEV)
    got, grad = _run(point, tri, torch.ones(2, 3, dtype=torch.float64), target_length=target)
    assert bool((grad == 0).all()) and bool((got[:, 0] == 0).all()) and bool((got[:, 2] == 0).all())
    assert float(got[0, 1]) == (0.0 if target is None else target ** 2)


@pytest.mark.parametrize("name", ["fan", "sphere12"])
def test_long_neighbour_lists(name):
    vertices, triangles, topo, dterms = _case(name)
    longest = max(len(n) for n in topo["neighbours"].values())
    assert longest == (71 if name == "fan" else 16)
    for target in (None, 0.2):
        want, want_grad = ref.gradients(vertices, topo, dterms, target_length=target)
        got, grad = _run(vertices, triangles.to(DEV), dterms, target_length=target)
        _check(got, grad, want, want_grad, "%s target %s" % (name, target))


def test_reduction_over_several_workgroups():
    vertices, triangles, topo, dterms = _case("sphere20")
    assert (vertices.shape[1], len(topo["edges"]), len(topo["flaps"])) == (402, 1203, 1197)
    want, want_grad = ref.gradients(vertices, topo, dterms)
    tri = triangles.to(DEV)
    got, grad = _run(vertices, tri, dterms)
    _check(got, grad, want, want_grad, "sphere K=20")
    for b in range(vertices.shape[0]):
        alone, alone_grad = _run(vertices[b:b + 1], tri, dterms[b:b + 1])
        assert torch.equal(alone[0], got[b]), "image %d: its terms depend on the rest of the batch" % b
        assert torch.equal(alone_grad[0], grad[b])


def test_bitwise_reproducible_in_either_mode():
    vertices, triangles, _, dterms = _case("sphere20")
    tri = triangles.to(DEV)
    before = _native.set_deterministic(False)
    try:
        runs = []
        for mode in (False, False, True, True):
            _native.set_deterministic(mode)
            runs.append(_run(vertices, tri, dterms, target_length=0.1))
    finally:
        _native.set_deterministic(before)
    for got, grad in runs[1:]:
        assert torch.equal(got, runs[0][0]) and torch.equal(grad, runs[0][1])


def test_captured_step_with_the_regulariser():
    vertices, triangles, normals = shapes.sphere(1.0, 6)
    B, V = 2, vertices.shape[0]
    tri = triangles.to(DEV)
    g = torch.Generator().manual_seed(4)
    v = (vertices[None] + 0.03 * torch.randn(B, V, 3, generator=g)).to(DEV).requires_grad_(True)
    normals = normals.to(DEV)[None].repeat(B, 1, 1)
    diffuse = torch.ones(B, V, 3, device=DEV)
    eye = torch.tensor([[0.0, 0.0, 3.0], [3.0, 0.0, 0.0]], device=DEV)
    center, up = torch.zeros(B, 3, device=DEV), torch.tensor([[0.0, 1.0, 0.0]] * B, device=DEV)
    lights, intensities = eye.unsqueeze(1).clone(), torch.ones(B, 1, 3, device=DEV)
    target = torch.rand(B, 48, 64, 4, generator=g).to(DEV)

    def loss_of(x):
        image = mesh_renderer.render(x, tri, normals, diffuse, eye, center, up, lights, intensities, 64, 48)
        return torch.mean(torch.abs(image - target)) + reg.mesh_regularizer(x, tri, 0.3, 0.2, 0.1).sum()

    def step():
        loss = loss_of(v)
        loss.backward()
        return loss

    captured = mesh_renderer.capture_step(step, [v])
    with torch.no_grad():
        v.add_(0.02 * torch.randn(B, V, 3, generator=g).to(DEV))
    loss = captured.replay().clone()
    grad = v.grad.clone()
    fresh = v.detach().clone().requires_grad_(True)
    eager = loss_of(fresh)
    eager.backward()
    assert abs(float(loss) - float(eager)) <= 1e-6 * abs(float(eager))
    assert float((grad - fresh.grad).abs().max()) <= 1e-6 * float(fresh.grad.abs().max())
    # the regulariser's part of the replayed gradient is the restatement's
    only = v.detach().clone().requires_grad_(True)
    reg.mesh_regularizer(only, tri, 0.3, 0.2, 0.1).sum().backward()
    weights = torch.tensor([[0.3, 0.2, 0.1]], dtype=torch.float64).repeat(B, 1)
    _, want_grad = ref.gradients(v.detach().cpu(), ref.topology(triangles, V), weights)
    assert float((only.grad.double().cpu() - want_grad).abs().max()) <= 1e-4 * float(want_grad.abs().max())


def test_regularised_fit_example():
    spec = importlib.util.spec_from_file_location("fit_mesh_regularized",
                                                  os.path.join(ROOT, "examples", "fit_mesh_regularized.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    losses, extent, terms = example.optimize(steps=100, size=64, resolution=10)
    plain_losses, plain_extent, plain_terms = example.optimize(steps=100, size=64, resolution=10, laplacian=0.0,
                                                               edge=0.0, normal=0.0)
    print("regularised: loss %.5f -> %.5f, extents %s, terms %s" % (losses[0], losses[-1], extent.tolist(),
                                                                      terms.tolist()))
    print("plain:       loss %.5f -> %.5f, extents %s, terms %s" % (plain_losses[0], plain_losses[-1],
                                                                      plain_extent.tolist(), plain_terms.tolist()))
    assert losses[-1] < losses[0] and plain_losses[-1] < plain_losses[0]
    assert abs(float(extent[0]) - 0.65) < abs(1.0 - 0.65)
    assert abs(float(extent[2]) - 0.8) < abs(1.0 - 0.8)
    assert float(terms[2]) < float(plain_terms[2]) and float(terms[0]) < float(plain_terms[0])
