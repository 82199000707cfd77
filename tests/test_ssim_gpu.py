"""The fused SSIM loss on the MI355X against its float64 restatement (tests/ssim_reference.py).

Budgets: the mean within 1e-5 absolute, the map within 5e-4 absolute, each gradient within 1e-4 of the largest
magnitude of the expected gradient tensor (the rule of test_regularizers_gpu.py).  A plain float32 eager torch
evaluation of the same formulas (blur(x^2) - mu^2) on these input families and windows stays within 8e-7 / 1.1e-4
(worst on the flat discs) / 2.1e-5 of float64, so the budgets leave room for another summation order and no more."""
import numpy as np
import pytest
import torch

import ssim_reference as ref
from conftest import bits_equal
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes
from pytorch_mesh_renderer_amd.mesh_renderer import losses
from pytorch_mesh_renderer_amd.mesh_renderer.rendered_image import RenderedImage

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SHAPES = [(2, 37, 45, 4), (1, 5, 70, 3), (1, 64, 64, 4), (1, 65, 33, 1), (3, 16, 17, 4), (1, 1, 1, 4)]
WINDOWS = [(11, 1.5), (7, 1.0), (3, 0.8)]
FAMILIES = {"noise": ref.noise_pair, "noisy_copy": ref.noisy_copy, "discs": ref.shaded_discs}
_cache = {}


def _inputs(family, shape):
    key = (family, shape)
    if key not in _cache:
        _cache[key] = FAMILIES[family](shape, seed=len(family) + sum(shape))
    return _cache[key]


def _expected(family, shape, window_size, sigma, padding, upstream=1.0):
    """The float64 restatement, computed once per case and shared."""
    key = (family, shape, window_size, sigma, padding, upstream)
    if key not in _cache:
        a, b = _inputs(family, shape)
        _cache[key] = ref.ssim_reference(a, b, window_size, sigma, padding, upstream=upstream)
    return _cache[key]


def _check_gradient(got, want, what):
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), what
    scale = float(np.abs(want).max())
    err = float(np.abs(got.double().cpu().numpy() - want).max())
    print("%s: gradient max err %.3g of scale %.3g (%.3g)" % (what, err, scale, err / max(scale, 1e-300)))
    assert err <= 1e-4 * scale, "%s: gradient error %.3g > 1e-4 * %.3g" % (what, err, scale)


def _paddings(shape, window_size):
    return ["same", "valid"] if min(shape[1], shape[2]) >= window_size else ["same"]


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "w%d" % w[0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_map_and_gradients_match_the_restatement(shape, window):
    window_size, sigma = window
    for family in FAMILIES:
        a_host, b_host = _inputs(family, shape)
        for padding in _paddings(shape, window_size):
            what = "%s %s w%d %s" % (family, shape, window_size, padding)
            want = _expected(family, shape, window_size, sigma, padding)
            a = torch.from_numpy(a_host).to(DEV).requires_grad_(True)
            b = torch.from_numpy(b_host).to(DEV).requires_grad_(True)
            value = losses.ssim(a, b, window_size=window_size, sigma=sigma, padding=padding)
            assert value.shape == () and value.dtype == torch.float32 and value.is_cuda
            value.backward()
            err = abs(float(value) - want["value"])
            print("%s: value %.7f err %.3g" % (what, float(value), err))
            assert err <= 1e-5, what
            _, got_map, _ = _native.ssim_forward(a.detach(), b.detach(), window_size, sigma, padding, 0.01 ** 2,
                                                 0.03 ** 2, want_map=True)
            assert tuple(got_map.shape) == want["map"].shape
            map_err = float(np.abs(got_map.double().cpu().numpy() - want["map"]).max())
            print("%s: map max err %.3g" % (what, map_err))
            assert map_err <= 5e-4, what
            _check_gradient(a.grad, want["dimage"], what + " d image")
            _check_gradient(b.grad, want["dtarget"], what + " d target")


def _eager_identical_gradient(image_host, window_size, sigma):
    """max |d ssim / d image| of the float32 eager spelling for image == target, on the CPU (the exact value is 0)."""
    x = torch.from_numpy(image_host).requires_grad_(True)
    ref.eager_float32_ssim(x, torch.from_numpy(image_host), window_size, sigma).backward()
    return float(x.grad.abs().max())


@pytest.mark.parametrize("family,shape", [("noise", (2, 37, 45, 4)), ("discs", (1, 64, 64, 4))])
def test_identical_images(family, shape):
    """ssim(x, x) is 1 and its gradient is exactly zero, so a relative bound has no meaning: the bound is ten times
    what the float32 eager spelling (grouped conv2d + autograd, on the CPU, computed here) leaves for the same input.
    Measured on the CPU for these inputs and the windows 11, 7, 3 -- noise 2x37x45x4: 2.2e-10, 1.6e-10, 2.6e-10 (a
    gradient between different images of that shape is of the order 1e-3); discs 1x64x64x4: 0, 0, 0, the eager
    cancellation happens to be exact there, which leaves the kernels no room at all: they form the terms so that
    identical images cancel exactly (csrc/ssim.hip, ssim_terms)."""
    image_host = _inputs(family, shape)[0]
    for window_size, sigma in WINDOWS:
        eager = _eager_identical_gradient(image_host, window_size, sigma)
        a = torch.from_numpy(image_host).to(DEV).requires_grad_(True)
        b = torch.from_numpy(image_host).to(DEV).requires_grad_(True)
        value = losses.ssim(a, b, window_size=window_size, sigma=sigma)
        value.backward()
        got = max(float(a.grad.abs().max()), float(b.grad.abs().max()))
        print("%s w%d: value - 1 = %.3g, gradient max %.3g, eager float32 %.3g" % (family, window_size,
                                                                                   float(value) - 1.0, got, eager))
        assert abs(float(value) - 1.0) <= 1e-6
        assert got <= 10.0 * eager


def _run(a_host, b_host, grad_a, grad_b, upstream=None, **kwargs):
    a = torch.from_numpy(a_host).to(DEV).requires_grad_(grad_a)
    b = torch.from_numpy(b_host).to(DEV).requires_grad_(grad_b)
    value = losses.ssim(a, b, **kwargs)
    (value if upstream is None else value * upstream).backward()
    return value.detach(), a.grad, b.grad


def test_gradient_to_either_input_alone_and_an_upstream_factor():
    shape, family = (2, 37, 45, 4), "noisy_copy"
    a_host, b_host = _inputs(family, shape)
    want = _expected(family, shape, 11, 1.5, "same", upstream=-2.5)
    calls = []
    before = _native.ssim_backward

    def spy(*args, **kwargs):
        out = before(*args, **kwargs)
        calls.append((out[0] is not None, out[1] is not None, int(args[2].numel())))
        return out
    _native.ssim_backward = spy
    try:
        plane = int(np.prod(shape))
        for grad_a, grad_b in ((True, False), (False, True), (True, True)):
            value, da, db = _run(a_host, b_host, grad_a, grad_b, upstream=-2.5)
            assert abs(float(value) - want["value"]) <= 1e-5
            assert (da is not None) == grad_a and (db is not None) == grad_b
            if grad_a:
                _check_gradient(da, want["dimage"], "upstream -2.5, d image (%s, %s)" % (grad_a, grad_b))
            if grad_b:
                _check_gradient(db, want["dtarget"], "upstream -2.5, d target (%s, %s)" % (grad_a, grad_b))
            # a gradient that is not required is not computed, and its plane is not saved
            assert calls[-1] == (grad_a, grad_b, (2 + grad_a + grad_b) * plane)
    finally:
        _native.ssim_backward = before
    # under no_grad nothing is saved, also for inputs that require a gradient (needs_input_grad ignores the grad mode)
    seen = []
    forward = _native.ssim_forward

    def spy_forward(*args, **kwargs):
        out = forward(*args, **kwargs)
        seen.append((kwargs.get("grads"), out[2]))
        return out
    _native.ssim_forward = spy_forward
    try:
        for requires in (False, True):
            with torch.no_grad():
                value = losses.ssim(torch.from_numpy(a_host).to(DEV).requires_grad_(requires),
                                    torch.from_numpy(b_host).to(DEV).requires_grad_(requires))
            assert abs(float(value) - _expected(family, shape, 11, 1.5, "same")["value"]) <= 1e-5
            assert not value.requires_grad and value.grad_fn is None
            assert seen[-1] == (0, None)
    finally:
        _native.ssim_forward = forward


def test_constants_follow_k1_k2_and_data_range():
    shape = (1, 64, 64, 4)
    a_host, b_host = _inputs("discs", shape)
    kwargs = dict(window_size=7, sigma=1.0, padding="valid", k1=0.02, k2=0.05, data_range=2.0)
    want = ref.ssim_reference(a_host, b_host, upstream=1.0, **kwargs)
    value, da, db = _run(a_host, b_host, True, True, **kwargs)
    assert abs(float(value) - want["value"]) <= 1e-5
    _check_gradient(da, want["dimage"], "k1, k2, data_range: d image")
    _check_gradient(db, want["dtarget"], "k1, k2, data_range: d target")


def test_non_contiguous_inputs():
    shape, family = (3, 16, 17, 4), "noise"
    a_host, b_host = _inputs(family, shape)
    want = _expected(family, shape, 7, 1.0, "same")
    a_leaf = torch.from_numpy(np.ascontiguousarray(a_host.transpose(0, 2, 1, 3))).to(DEV).requires_grad_(True)
    wide = torch.zeros(3, 16, 17, 8, device=DEV)
    wide[..., ::2] = torch.from_numpy(b_host).to(DEV)
    b_leaf = wide.requires_grad_(True)
    a, b = a_leaf.permute(0, 2, 1, 3), b_leaf[..., ::2]
    assert not a.is_contiguous() and not b.is_contiguous()
    value = losses.ssim(a, b, window_size=7, sigma=1.0)
    value.backward()
    assert abs(float(value) - want["value"]) <= 1e-5
    _check_gradient(a_leaf.grad.permute(0, 2, 1, 3), want["dimage"], "permuted image")
    _check_gradient(b_leaf.grad[..., ::2], want["dtarget"], "strided target")
    assert float(b_leaf.grad[..., 1::2].abs().max()) == 0.0


def test_results_are_bitwise_reproducible():
    assert not _native.deterministic()
    shape = (2, 37, 45, 4)
    a_host, b_host = _inputs("noisy_copy", shape)
    runs = []
    for _ in range(2):
        value, da, db = _run(a_host, b_host, True, True)
        a, b = torch.from_numpy(a_host).to(DEV), torch.from_numpy(b_host).to(DEV)
        _, ssim_map, _ = _native.ssim_forward(a, b, want_map=True)
        runs.append([t.cpu().numpy() for t in (value, ssim_map, da, db)])
    for name, first, second in zip(("value", "map", "d image", "d target"), *runs):
        assert bits_equal(first, second), name
    assert float(np.abs(runs[0][2]).max()) > 0


def test_forward_and_backward_are_capturable_into_a_hip_graph():
    shape = (2, 37, 45, 4)
    a_host, b_host = _inputs("noise", shape)
    a = torch.from_numpy(a_host).to(DEV).requires_grad_(True)
    b = torch.from_numpy(b_host).to(DEV).requires_grad_(True)

    def step():
        value = losses.ssim(a, b)
        value.backward()
        return value
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            a.grad = b.grad = None
            step()
    torch.cuda.current_stream().wait_stream(side)
    a.grad = b.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        value = step()
    new_a, new_b = _inputs("noisy_copy", shape)
    with torch.no_grad():
        a.copy_(torch.from_numpy(new_a).to(DEV))
        b.copy_(torch.from_numpy(new_b).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone().cpu().numpy() for t in (value.detach(), a.grad, b.grad)]
    want_value, want_da, want_db = _run(new_a, new_b, True, True)
    for name, g, w in zip(("value", "d image", "d target"), got, (want_value, want_da, want_db)):
        assert bits_equal(g, w.cpu().numpy()), name
    assert abs(float(got[0]) - _expected("noisy_copy", shape, 11, 1.5, "same")["value"]) <= 1e-5


def _cube_scene():
    vertices, triangles, normals = shapes.cube(2.0)
    triangles = torch.flip(triangles, [1]).contiguous().to(DEV)
    eye = torch.tensor([[2.0, 3.0, 6.0]])
    diffuse = torch.rand(1, 8, 3, generator=torch.Generator().manual_seed(11)) * 0.6 + 0.3

    def render(v, kd):
        return mesh_renderer.render(v, triangles, normals.unsqueeze(0).to(DEV), kd, eye.to(DEV),
                                    torch.zeros(1, 3, device=DEV), torch.tensor([[0.0, 1.0, 0.0]], device=DEV),
                                    eye.unsqueeze(1).to(DEV), torch.ones(1, 1, 3, device=DEV), 64, 48)
    leaves = lambda: (vertices.unsqueeze(0).clone().to(DEV).requires_grad_(True),
                      diffuse.clone().to(DEV).requires_grad_(True))
    with torch.no_grad():
        v, kd = leaves()
        target = render(v * 0.93, kd.flip(1)).detach().as_subclass(torch.Tensor).roll(2, 2).contiguous()
    return render, leaves, target


@pytest.mark.parametrize("weight", [0.2, 0.0, 1.0])
def test_photometric_loss_on_renders_own_output(weight):
    """(1 - w) l1 + w (1 - ssim) on render()'s direct output (fused L1 route + the SSIM gradient through the renderer's
    node) against the same expression on a detached-and-reattached copy of the image (generic routes), value and the
    gradients of the vertices and the diffuse colours, 1e-4 of scale."""
    render, leaves, target = _cube_scene()
    v, kd = leaves()
    image = render(v, kd)
    assert isinstance(image, RenderedImage) and tuple(image.shape) == (1, 48, 64, 4)
    loss = losses.photometric_loss(image, target, ssim_weight=weight)
    loss.backward()

    v2, kd2 = leaves()
    image2 = render(v2, kd2)
    copy = image2.detach().as_subclass(torch.Tensor).clone().requires_grad_(True)
    want = (1.0 - weight) * losses._MeanAbsError.apply(copy, target) + weight * (1.0 - losses.ssim(copy, target))
    want.backward()
    image2.backward(copy.grad)
    truth = ref.ssim_reference(copy.detach().cpu().numpy(), target.cpu().numpy())["value"]
    truth = (1.0 - weight) * float((copy.detach().double() - target.double()).abs().mean()) + weight * (1.0 - truth)
    print("w = %.1f: loss %.7f, generic %.7f, float64 %.7f" % (weight, float(loss), float(want), truth))
    assert abs(float(loss) - float(want)) <= 1e-4 * abs(float(want))
    assert abs(float(loss) - truth) <= 1e-5
    for name, got, expected in (("d vertices", v.grad, v2.grad), ("d diffuse", kd.grad, kd2.grad)):
        scale = float(expected.abs().max())
        err = float((got - expected).abs().max())
        print("w = %.1f %s: max err %.3g of scale %.3g" % (weight, name, err, scale))
        assert scale > 0 and err <= 1e-4 * scale, name


def test_a_rendered_image_is_accepted_like_a_plain_tensor():
    render, leaves, target = _cube_scene()
    v, kd = leaves()
    image = render(v, kd)
    assert isinstance(image, RenderedImage)
    value = losses.ssim(image, target, window_size=7, sigma=1.0)
    value.backward()
    want = ref.ssim_reference(image.detach().cpu().numpy(), target.cpu().numpy(), 7, 1.0)
    assert abs(float(value) - want["value"]) <= 1e-5
    v2, kd2 = leaves()
    image2 = render(v2, kd2)
    image2.backward(torch.from_numpy(want["dimage"]).float().to(DEV))
    for name, got, expected in (("d vertices", v.grad, v2.grad), ("d diffuse", kd.grad, kd2.grad)):
        scale = float(expected.abs().max())
        assert scale > 0 and float((got - expected).abs().max()) <= 1e-4 * scale, name
