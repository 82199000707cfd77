"""Silhouette antialiasing on the MI355X against its restatement (tests/antialias_reference.py)."""
import importlib

import numpy as np
import pytest
import torch

import antialias_reference as ref
from antialias_scenes import CUBE_EYES, _cube_clip, _soup
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import camera_utils, shapes, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _gbuffer(clip, tris, width, height):
    ids, bary, z = _native.rasterize_forward(clip.to(DEV), tris.to(DEV), width, height)
    return ids, bary, z


def _compare(clip, tris, width, height, C, seed=0):
    """Kernel forward + backward against the restatement on one scene; returns the restatement's pairs."""
    ids, bary, z = _gbuffer(clip, tris, width, height)
    g = torch.Generator().manual_seed(seed)
    B = clip.shape[0]
    image = torch.rand(B, height, width, C, generator=g)
    dout = torch.randn(B, height, width, C, generator=g)
    opp = mesh_renderer.antialias_topology(tris.to(DEV), clip.shape[1])
    np.testing.assert_array_equal(opp.cpu().numpy(), ref.topology(tris.numpy(), clip.shape[1]))
    out, mask = _native.antialias_forward(image.to(DEV), ids, bary, z, clip.to(DEV), tris.to(DEV), opp,
                                          want_pair_mask=True)
    pairs, want_mask = ref.decide(ids.cpu().numpy(), bary.cpu().numpy(), z.cpu().numpy(), clip.numpy(),
                                  tris.numpy(), opp.cpu().numpy())
    got_mask = mask.cpu().numpy()
    assert np.array_equal(got_mask, want_mask), "blended pairs differ at %d pixels" % int((got_mask != want_mask).sum())
    img64 = image.double().requires_grad_(True)
    clip64 = clip.double().requires_grad_(True)
    want = ref.antialias(img64, clip64, pairs)
    assert float((out.cpu().double() - want.detach()).abs().max()) <= 1e-6
    (want * dout.double()).sum().backward()
    x = clip.to(DEV).requires_grad_(True)
    im = image.to(DEV).requires_grad_(True)
    y = mesh_renderer.antialias(im, x, tris.to(DEV), ids, bary, z)
    assert torch.equal(y.detach(), out)
    y.backward(dout.to(DEV))
    assert float((im.grad.cpu().double() - img64.grad).abs().max()) <= 1e-6
    ref_dclip = clip64.grad
    tol = 1e-4 * float(ref_dclip.abs().max()) + 1e-7
    assert float((x.grad.cpu().double() - ref_dclip).abs().max()) <= tol
    return pairs, ids


@pytest.mark.parametrize("cam", range(4))
def test_cube_matches_the_restatement(cam):
    clip, tris = _cube_clip(CUBE_EYES[cam:cam + 1], 64, 48)
    pairs, _ = _compare(clip, tris, 64, 48, 4, seed=cam)
    assert len(pairs["t"]) > 20


def test_sphere_5k_256_batch_8_matches_the_restatement():
    job = synthetic.sphere_job(8, 256, 256)
    pairs, _ = _compare(job["clip"], job["triangles"], 256, 256, 4)
    assert len(pairs["t"]) > 1000


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_triangle_soups_match_the_restatement(seed):
    clip, tris = _soup(seed)
    pairs, _ = _compare(clip, tris, 96, 80, 3, seed=seed)
    assert len(pairs["t"]) > 50


@pytest.mark.parametrize("C", [1, 3, 4, 7])
def test_every_channel_count(C):
    clip, tris = _cube_clip(CUBE_EYES[:2], 64, 48)
    _compare(clip, tris, 64, 48, C, seed=C)


def test_constant_image_is_unchanged_and_has_no_vertex_gradient():
    job = synthetic.sphere_job(2, 128, 96)
    clip, tris = job["clip"].to(DEV), job["triangles"].to(DEV)
    ids, bary, z = _gbuffer(clip, tris, 128, 96)
    image = torch.full((2, 96, 128, 4), 0.375, device=DEV, requires_grad=True)
    x = clip.clone().requires_grad_(True)
    out = mesh_renderer.antialias(image, x, tris, ids, bary, z)
    assert torch.equal(out.detach(), image.detach())
    out.backward(torch.randn_like(out))
    assert float(x.grad.abs().max()) == 0.0


def test_closed_cube_blends_only_its_outline():
    for cam in range(4):
        clip, tris = _cube_clip(CUBE_EYES[cam:cam + 1], 64, 48)
        ids, bary, z = _gbuffer(clip, tris, 64, 48)
        cov = ((ids != 0) | (bary.sum(-1) >= 0.9)).cpu().numpy()
        pairs, _ = ref.decide(ids.cpu().numpy(), bary.cpu().numpy(), z.cpu().numpy(), clip.numpy(), tris.numpy(),
                              ref.topology(tris.numpy(), 8))
        b = pairs["b"]
        assert len(b) > 0
        assert np.all(cov[b, pairs["fy"], pairs["fx"]] != cov[b, pairs["gy"], pairs["gx"]])


def test_batched_equals_per_image():
    job = synthetic.sphere_job(3, 128, 96)
    clip, tris = job["clip"].to(DEV), job["triangles"].to(DEV)
    ids, bary, z = _gbuffer(clip, tris, 128, 96)
    g = torch.Generator().manual_seed(5)
    image = torch.rand(3, 96, 128, 4, generator=g).to(DEV)
    dout = torch.randn(3, 96, 128, 4, generator=g).to(DEV)
    opp = mesh_renderer.antialias_topology(tris, clip.shape[1])
    out = _native.antialias_forward(image, ids, bary, z, clip, tris, opp)
    dimage, dclip = _native.antialias_backward(dout, image, ids, bary, z, clip, tris, opp)
    for b in range(3):
        s = slice(b, b + 1)
        o = _native.antialias_forward(image[s], ids[s], bary[s], z[s], clip[s], tris, opp)
        di, dc = _native.antialias_backward(dout[s], image[s], ids[s], bary[s], z[s], clip[s], tris, opp)
        assert torch.equal(o, out[s]) and torch.equal(di, dimage[s])
        before = _native.set_deterministic(True)
        try:
            dc_det = _native.antialias_backward(dout[s], image[s], ids[s], bary[s], z[s], clip[s], tris, opp)[1]
            all_det = _native.antialias_backward(dout, image, ids, bary, z, clip, tris, opp)[1]
        finally:
            _native.set_deterministic(before)
        assert torch.allclose(dc, dclip[s], rtol=1e-5, atol=1e-6)
        assert torch.allclose(dc_det, all_det[s], rtol=1e-5, atol=1e-6)


def test_deterministic_mode_reproduces_dclip_bit_for_bit():
    job = synthetic.sphere_job(8, 256, 256)
    clip, tris = job["clip"].to(DEV), job["triangles"].to(DEV)
    ids, bary, z = _gbuffer(clip, tris, 256, 256)
    g = torch.Generator().manual_seed(7)
    image = torch.rand(8, 256, 256, 4, generator=g).to(DEV)
    dout = torch.randn(8, 256, 256, 4, generator=g).to(DEV)
    opp = mesh_renderer.antialias_topology(tris, clip.shape[1])
    float_dclip = _native.antialias_backward(dout, image, ids, bary, z, clip, tris, opp)[1]
    before = _native.set_deterministic(True)
    try:
        runs = [_native.antialias_backward(dout, image, ids, bary, z, clip, tris, opp) for _ in range(2)]
        # a contribution outside the fixed-point range (csrc/det_fixed.h) -- an infinite upstream gradient on one
        # pixel that a blended pair modifies, and a NaN -- poisons the whole of dclip (dimage is written per pixel)
        pair_mask = _native.antialias_forward(image, ids, bary, z, clip, tris, opp, want_pair_mask=True)[1]
        blended = (pair_mask != 0).nonzero()
        b, y, x = [int(t) for t in blended[len(blended) // 2]]
        for poison in (float("inf"), float("nan")):
            bad = dout.clone()
            bad[b, y, x, 1] = poison
            poisoned = _native.antialias_backward(bad, image, ids, bary, z, clip, tris, opp)[1]
            assert not bool(torch.isfinite(poisoned).any()), poison
    finally:
        _native.set_deterministic(before)
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][0], runs[1][0])
    assert float(runs[0][1].abs().max()) > 0
    tol = 1e-5 * float(float_dclip.abs().max())
    assert float((runs[0][1] - float_dclip).abs().max()) <= tol


def _render_scene(vertices, antialias, width=64, height=48):
    _, tris, normals = shapes.cube(2.0)
    tris = torch.flip(tris, [1]).contiguous().to(DEV)
    eye = torch.tensor([[2.0, 3.0, 6.0]], device=DEV)
    return mesh_renderer.render(vertices, tris, normals.unsqueeze(0).to(DEV), torch.ones(1, 8, 3, device=DEV) * 0.8,
                                eye, torch.zeros(1, 3, device=DEV), torch.tensor([[0.0, 1.0, 0.0]], device=DEV),
                                eye.unsqueeze(1), torch.ones(1, 1, 3, device=DEV), width, height,
                                antialias=antialias)


def test_render_antialias_equals_the_composed_construction():
    render_module = importlib.import_module("pytorch_mesh_renderer_amd.mesh_renderer.render")
    from pytorch_mesh_renderer_amd.mesh_renderer.rasterize_triangles_ext import (AttributeInterpolator,
                                                                                  BarycentricRasterizer)
    vertices, tris, normals = shapes.cube(2.0)
    vertices = vertices.unsqueeze(0).to(DEV)
    got = _render_scene(vertices, True)
    tris = torch.flip(tris, [1]).contiguous().to(DEV)
    eye = torch.tensor([[2.0, 3.0, 6.0]], device=DEV)
    transforms = camera_utils.clip_space_transforms(eye, torch.zeros(1, 3, device=DEV),
                                                    torch.tensor([[0.0, 1.0, 0.0]], device=DEV),
                                                    torch.full((1,), 40.0, device=DEV), torch.full((1,), 0.01, device=DEV),
                                                    torch.full((1,), 10.0, device=DEV), 64 / 48, DEV)
    clip = camera_utils.transform_homogeneous(transforms, vertices)
    ids, bary, z = BarycentricRasterizer.apply(clip, tris, 64, 48)
    diffuse = torch.ones(1, 8, 3, device=DEV) * 0.8
    attrs = torch.cat([normals.unsqueeze(0).to(DEV), vertices, diffuse], 2)
    px = AttributeInterpolator.apply(ids, bary, attrs, tris, torch.full((9,), -1.0, device=DEV))
    rgba = render_module._phong_rgba(torch.nn.functional.normalize(px[..., 0:3], p=2, dim=3),
                                     (px[..., 6:9] >= 0).any(dim=3).to(torch.float32), px[..., 3:6],
                                     eye.unsqueeze(1), torch.ones(1, 1, 3, device=DEV), px[..., 6:9])
    want = torch.flip(mesh_renderer.antialias(rgba, clip, tris, ids, bary, z), dims=[1])
    assert torch.equal(got, want)
    plain = _render_scene(vertices, False)
    assert torch.equal(plain, mesh_renderer.render(*_render_args(vertices)))
    alpha = got[..., 3]
    assert ((alpha > 0) & (alpha < 1)).any()      # fractional on the outline


def _render_args(vertices):
    _, tris, normals = shapes.cube(2.0)
    tris = torch.flip(tris, [1]).contiguous().to(DEV)
    eye = torch.tensor([[2.0, 3.0, 6.0]], device=DEV)
    return (vertices, tris, normals.unsqueeze(0).to(DEV), torch.ones(1, 8, 3, device=DEV) * 0.8, eye,
            torch.zeros(1, 3, device=DEV), torch.tensor([[0.0, 1.0, 0.0]], device=DEV), eye.unsqueeze(1),
            torch.ones(1, 1, 3, device=DEV), 64, 48)


def test_alpha_loss_has_a_vertex_gradient_only_with_antialiasing():
    vertices, _, _ = shapes.cube(2.0)
    grads = []
    for aa in (False, True):
        v = vertices.unsqueeze(0).to(DEV).clone().requires_grad_(True)
        _render_scene(v, aa)[..., 3].sum().backward()
        grads.append(v.grad)
    assert float(grads[0].abs().max()) == 0.0
    assert float(grads[1].abs().max()) > 0.0


def test_example_recovers_an_offset():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fit_silhouette_antialiased",
                                                  os.path.join(root, "examples", "fit_silhouette_antialiased.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    result = example.fit(steps=150, device=DEV)
    assert result["error_px"] < 0.05, result


def test_antialiased_step_replays_bit_identically_under_capture():
    """rasterize -> antialias -> loss -> backward as one captured graph: with set_deterministic(True) every
    gradient of the step is order-free, so each replay equals the eager step bit for bit."""
    from pytorch_mesh_renderer_amd.mesh_renderer.rasterize_triangles_ext import BarycentricRasterizer
    job = synthetic.sphere_job(2, 128, 96)
    clip = job["clip"].to(DEV).requires_grad_(True)
    tris = job["triangles"].to(DEV)
    opp = mesh_renderer.antialias_topology(tris, clip.shape[1])
    g = torch.Generator().manual_seed(11)
    colour = torch.rand(2, 96, 128, 4, generator=g).to(DEV).requires_grad_(True)
    target = torch.rand(2, 96, 128, 4, generator=g).to(DEV)

    def step():
        ids, bary, z = BarycentricRasterizer.apply(clip, tris, 128, 96)
        image = mesh_renderer.antialias(colour * bary.sum(-1, keepdim=True), clip, tris, ids, bary, z, opp)
        loss = torch.mean((image - target) ** 2)
        loss.backward()
        return loss

    before = _native.set_deterministic(True)
    try:
        clip.grad = colour.grad = None
        eager_loss = step().detach().clone()
        eager = (clip.grad.clone(), colour.grad.clone())
        assert float(eager[0].abs().max()) > 0
        captured = mesh_renderer.capture_step(step, [clip, colour])
        for _ in range(2):
            loss = captured.replay()
            torch.cuda.synchronize()
            assert torch.equal(loss, eager_loss)
            assert torch.equal(clip.grad, eager[0]) and torch.equal(colour.grad, eager[1])
    finally:
        _native.set_deterministic(before)
