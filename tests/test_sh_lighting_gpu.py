"""Spherical-harmonics lighting on the MI355X against its restatement (tests/sh_reference.py) and against the
package's torch path (sh_lighting.USE_SH_KERNELS = False)."""
import importlib
import importlib.util
import itertools
import os

import pytest
import torch

import sh_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
sh_lighting = importlib.import_module("pytorch_mesh_renderer_amd.mesh_renderer.sh_lighting")


def _buffers(B, H, W, seed, device=DEV):
    """Random pixel buffers: normals of length 0.5..2 with some exactly zero, diffuse colours with background
    pixels (-1), alphas among {0, 0.3, 0.5, 0.7, 1}, coefficients, and an upstream gradient."""
    g = torch.Generator().manual_seed(seed)
    normals = torch.randn(B, H, W, 3, generator=g)
    normals = normals / normals.norm(dim=-1, keepdim=True).clamp(min=1e-3) * (0.5 + 1.5 * torch.rand(B, H, W, 1, generator=g))
    normals[torch.rand(B, H, W, generator=g) < 0.05] = 0.0
    diffuse = torch.rand(B, H, W, 3, generator=g)
    diffuse[torch.rand(B, H, W, generator=g) < 0.2] = -1.0
    alphas = torch.tensor([0.0, 0.3, 0.5, 0.7, 1.0])[torch.randint(0, 5, (B, H, W), generator=g)]
    sh = torch.randn(B, 9, 3, generator=g) * 0.5
    drgba = torch.randn(B, H, W, 4, generator=g)
    return [t.to(device) for t in (normals, diffuse, alphas, sh, drgba)]


def _lay_out(normals, diffuse, stride):
    """stride 3: two buffers; stride 6: two channel slices of one packed buffer (read in place)."""
    if stride == 3:
        return normals.contiguous(), diffuse.contiguous()
    packed = torch.cat([normals, diffuse], -1).contiguous()
    return packed[..., 0:3], packed[..., 3:6]


def _close(got, want, tol, what):
    err = float((got.detach().double() - want).abs().max()) if got.numel() else 0.0
    assert err <= tol, "%s: max |error| %.3g > %.3g" % (what, err, tol)


def _pixel_grad_ok(got, want, what):
    """per-pixel gradients within 1e-5, relative to the pixel's largest component where that exceeds 1: a
    zero-length normal's gradient is a three-term sum divided by the 1e-12 floor, so one of its components can be
    a float32 cancellation of numbers 1e12 times larger than 1"""
    scale = want.abs().amax(dim=-1, keepdim=True).clamp(min=1.0)
    err = (got.double() - want).abs() / scale
    assert float(err.max()) <= 1e-5, "%s: max scaled error %.3g" % (what, float(err.max()))


def _check_case(B, H, W, stride, flip, with_alphas, seed):
    normals, diffuse, alphas, sh, drgba = _buffers(B, H, W, seed)
    alphas = alphas if with_alphas else None
    n_in, d_in = _lay_out(normals, diffuse, stride)
    if stride == 6:
        assert _native._pixel_stride(n_in, d_in) == (6, 0, 3)
    rgba = _native.sh_shade_forward(n_in, d_in, alphas, sh, flip=flip)
    want = ref.shade(normals, diffuse, alphas, sh, flip=flip)
    _close(rgba, want, 1e-5, "rgba")
    grads = ref.gradients(normals, diffuse, alphas, sh, drgba, flip=flip)
    scale = ref.dsh_abs_terms(normals, diffuse, alphas, drgba, flip=flip)
    for wn, wd, wa, ws in itertools.product((False, True), repeat=4):
        dn, dd, da, dsh = _native.sh_shade_backward(drgba, n_in, d_in, alphas, sh, flip=flip, want_normals=wn,
                                                    want_diffuse=wd, want_alphas=wa, want_sh=ws)
        assert (dn is not None) == wn and (dd is not None) == wd and (dsh is not None) == ws
        assert (da is not None) == (wa and with_alphas)
        if wn:
            _pixel_grad_ok(dn, grads["normals"], "dnormals")
        if wd:
            _pixel_grad_ok(dd, grads["diffuse"], "ddiffuse")
        if da is not None:
            _close(da, grads["alphas"], 0.0, "dalphas")
        if ws:
            excess = (dsh.double() - grads["sh"]).abs() - 1e-4 * scale
            assert float(excess.max()) <= 1e-12, "dsh beyond 1e-4 of its terms' magnitude"
    # every output of the buffer path is written: masked pixels get exact zeros
    dn, dd, _, _ = _native.sh_shade_backward(drgba, n_in, d_in, alphas, sh, flip=flip)
    mask = (alphas if with_alphas else (diffuse >= 0).any(-1).float()) <= 0.5
    assert bool((dn[mask] == 0).all()) and bool((dd[mask] == 0).all())


@pytest.mark.parametrize("B, H, W", [(3, 17, 70), (2, 1, 129), (1, 33, 1), (3, 48, 64), (1, 1, 1)])
@pytest.mark.parametrize("stride", [3, 6])
@pytest.mark.parametrize("flip", [True, False])
def test_buffers_match_the_restatement(B, H, W, stride, flip):
    _check_case(B, H, W, stride, flip, with_alphas=True, seed=B * 1000 + H * 10 + W)


@pytest.mark.parametrize("stride", [3, 6])
@pytest.mark.parametrize("flip", [True, False])
def test_derived_alpha_matches_the_restatement(stride, flip):
    _check_case(3, 37, 91, stride, flip, with_alphas=False, seed=stride + 10 * flip)


def test_sh_shader_autograd_matches_the_restatement():
    normals, diffuse, alphas, sh, drgba = _buffers(2, 40, 50, 7)
    leaves = [t.clone().requires_grad_(True) for t in (normals, alphas, diffuse)]
    shared = sh[0].clone().requires_grad_(True)
    out = mesh_renderer.sh_shader(leaves[0], leaves[1], leaves[2], shared)
    _close(out, ref.shade(normals, diffuse, alphas, sh[0].expand(2, 9, 3)), 1e-5, "rgba")
    out.backward(drgba)
    grads = ref.gradients(normals, diffuse, alphas, sh[0].expand(2, 9, 3).contiguous(), drgba)
    _pixel_grad_ok(leaves[0].grad, grads["normals"], "normals")
    _close(leaves[1].grad, grads["alphas"], 0.0, "alphas")
    _pixel_grad_ok(leaves[2].grad, grads["diffuse"], "diffuse")
    scale = ref.dsh_abs_terms(normals, diffuse, alphas, drgba).sum(0)
    assert float(((shared.grad.double() - grads["sh"].sum(0)).abs() - 1e-4 * scale).max()) <= 1e-12


def test_full_size_workspace_reduction():
    """1024^2 x 32, packed stride 6: the dsh rows of 1024 workgroups per image and their sum."""
    B, S = 32, 1024
    g = torch.Generator(device=DEV).manual_seed(3)
    packed = torch.rand(B, S, S, 6, generator=g, device=DEV) * 2.0 - 0.5
    sh = torch.randn(B, 9, 3, generator=g, device=DEV)
    drgba = torch.randn(B, S, S, 4, generator=g, device=DEV)
    n_in, d_in = packed[..., 0:3], packed[..., 3:6]
    rgba = _native.sh_shade_forward(n_in, d_in, None, sh)
    dpacked, _, dsh = _native.sh_shade_backward(drgba, n_in, d_in, None, sh, packed_grad=True)
    for b in (0, 17, 31):
        want = ref.shade(n_in[b:b + 1], d_in[b:b + 1], None, sh[b:b + 1])
        _close(rgba[b:b + 1], want, 1e-5, "rgba")
    grads = ref.gradients(n_in, d_in, None, sh, drgba)
    scale = ref.dsh_abs_terms(n_in, d_in, None, drgba)
    assert float(((dsh.double() - grads["sh"]).abs() - 1e-4 * scale).max()) <= 1e-12
    for b in (0, 31):
        _pixel_grad_ok(dpacked[b, ..., 0:3], grads["normals"][b], "dnormals")
        _pixel_grad_ok(dpacked[b, ..., 3:6], grads["diffuse"][b], "ddiffuse")


# ---- render_sh ---------------------------------------------------------------------------------------------------
def _sh_target(device=DEV):
    return torch.tensor([[0.9, 0.8, 0.7], [0.2, 0.1, 0.0], [0.4, 0.45, 0.5], [-0.1, 0.05, 0.2], [0.05, -0.05, 0.0],
                         [0.1, 0.0, -0.1], [-0.15, -0.1, -0.05], [0.0, 0.1, 0.05], [0.08, 0.0, -0.08]], device=device)


def _scene(mesh, B=2, width=96, height=72):
    if mesh == "cube":
        vertices, triangles, normals = shapes.cube(2.0)
        triangles = torch.flip(triangles, [1]).contiguous()
    else:
        vertices, triangles, normals = shapes.sphere(1.0, 50)
    V = vertices.shape[0]
    g = torch.Generator().manual_seed(V)
    eyes = torch.tensor([[2.0, 3.0, 6.0], [-4.0, 1.0, 4.5], [0.3, -2.0, 5.0]])[:B] * (0.6 if mesh == "sphere" else 1.0)
    return {"vertices": vertices.unsqueeze(0).repeat(B, 1, 1).to(DEV), "triangles": triangles.to(DEV),
            "normals": normals.unsqueeze(0).repeat(B, 1, 1).to(DEV),
            "diffuse": (0.3 + 0.7 * torch.rand(B, V, 3, generator=g)).to(DEV),
            "sh": (_sh_target().unsqueeze(0) + 0.05 * torch.randn(B, 9, 3, generator=g).to(DEV)),
            "eye": eyes.to(DEV), "width": width, "height": height}


def _render_grads(scene, antialias, kernels, drgba=None):
    saved = sh_lighting.USE_SH_KERNELS
    sh_lighting.USE_SH_KERNELS = kernels
    try:
        leaves = {k: scene[k].clone().requires_grad_(True) for k in ("vertices", "normals", "diffuse", "sh")}
        B = scene["eye"].shape[0]
        image = mesh_renderer.render_sh(leaves["vertices"], scene["triangles"], leaves["normals"], leaves["diffuse"],
                                        leaves["sh"], scene["eye"], torch.zeros(B, 3, device=DEV),
                                        torch.tensor([0.0, 1.0, 0.0], device=DEV), scene["width"], scene["height"],
                                        antialias=antialias)
        if drgba is None:
            drgba = torch.randn(image.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
        (image * drgba).sum().backward()
        return image.detach(), {k: v.grad for k, v in leaves.items()}, drgba
    finally:
        sh_lighting.USE_SH_KERNELS = saved


@pytest.mark.parametrize("mesh", ["cube", "sphere"])
@pytest.mark.parametrize("antialias", [False, True])
def test_render_sh_matches_the_torch_path(mesh, antialias):
    scene = _scene(mesh)
    image, grads, drgba = _render_grads(scene, antialias, True)
    want_image, want_grads, _ = _render_grads(scene, antialias, False, drgba)
    covered = image[..., 3] > 0
    assert 0.05 < float(covered.float().mean()) < 0.95
    if antialias:
        assert bool(((image[..., 3] > 0) & (image[..., 3] < 1)).any())
    _close(image, want_image.double(), 1e-5, "rgba")
    for name in ("vertices", "normals", "diffuse", "sh"):
        tol = 1e-4 * float(want_grads[name].abs().max())
        assert tol > 0, name
        _close(grads[name], want_grads[name].double(), tol, name)


def test_render_sh_with_shared_coefficients_and_host_cameras():
    scene = _scene("cube", B=3)
    shared = _sh_target().clone().requires_grad_(True)
    center, up = torch.zeros(3, device=DEV), torch.tensor([0.0, 1.0, 0.0], device=DEV)
    args = (scene["vertices"], scene["triangles"], scene["normals"], scene["diffuse"])
    image = mesh_renderer.render_sh(*args, shared, scene["eye"], center, up, 64, 48)
    per_image = mesh_renderer.render_sh(*args, shared.detach().expand(3, 9, 3).contiguous(), scene["eye"], center, up,
                                        64, 48)
    assert torch.equal(image.detach(), per_image)
    image[..., :3].sum().backward()
    assert shared.grad.shape == (9, 3) and float(shared.grad.abs().max()) > 0
    host = mesh_renderer.render_sh(*args, shared.detach(), scene["eye"].cpu(), center.cpu(), up.cpu(), 64, 48)
    assert host.shape == (3, 48, 64, 4) and host.device == DEV
    assert float((host[..., 3] != per_image[..., 3]).float().mean()) < 0.01


def _shader_run(seed=21):
    normals, diffuse, alphas, sh, drgba = _buffers(3, 130, 257, seed)
    leaves = [t.clone().requires_grad_(True) for t in (normals, alphas, diffuse, sh)]
    out = mesh_renderer.sh_shader(*leaves)
    out.backward(drgba)
    return [out.detach()] + [t.grad for t in leaves]


def test_bit_identical_runs_with_and_without_deterministic_mode():
    first, second = _shader_run(), _shader_run()
    before = _native.set_deterministic(True)
    try:
        third = _shader_run()
        scene = _scene("sphere")
        runs = [_render_grads(scene, False, True) for _ in range(2)]
    finally:
        _native.set_deterministic(before)
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(runs[0][0], runs[1][0])
    for name in ("vertices", "normals", "diffuse", "sh"):
        assert torch.equal(runs[0][1][name], runs[1][1][name]), name


def test_captured_step_replays_to_the_eager_result():
    scene = _scene("sphere")
    vertices = scene["vertices"].clone().requires_grad_(True)
    sh = scene["sh"].clone().requires_grad_(True)
    target = torch.rand(2, scene["height"], scene["width"], 4, generator=torch.Generator().manual_seed(4)).to(DEV)
    center, up = torch.zeros(2, 3, device=DEV), torch.tensor([[0.0, 1.0, 0.0]], device=DEV).repeat(2, 1)

    def step():
        image = mesh_renderer.render_sh(vertices, scene["triangles"], scene["normals"], scene["diffuse"], sh,
                                        scene["eye"], center, up, scene["width"], scene["height"])
        loss = torch.mean(torch.abs(image - target))
        loss.backward()
        return loss

    before = _native.set_deterministic(True)
    try:
        vertices.grad = sh.grad = None
        eager_loss = step().detach().clone()
        eager = (vertices.grad.clone(), sh.grad.clone())
        assert float(eager[0].abs().max()) > 0 and float(eager[1].abs().max()) > 0
        captured = mesh_renderer.capture_step(step, [vertices, sh])
        for _ in range(2):
            loss = captured.replay()
            torch.cuda.synchronize()
            assert torch.equal(loss, eager_loss)
            assert torch.equal(vertices.grad, eager[0]) and torch.equal(sh.grad, eager[1])
    finally:
        _native.set_deterministic(before)


def test_example_recovers_the_lighting():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fit_sh_lighting", os.path.join(root, "examples", "fit_sh_lighting.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    result = example.fit(steps=300, size=64, device=DEV)
    assert result["final_loss"] <= 1e-3 * result["initial_loss"], result
    assert result["coefficient_error"] <= 1e-2, result
