"""The private G-buffer of the loss-in-forward route (mr_render_forward_l1_private, rasterize_triangles_ext.private_gbuffer):
no barycentric plane, id -1 on background, barycentrics rebuilt in the backward's lane kernel (ShadeFoldLaneNoBaryFn).
The yardstick is the same scene with the switch off:
  image, sign codes, empty map   torch.equal (bit patterns)
  ids                            equal after -1 -> 0
  loss                           equal (the same partial sums in the same order)
  vertex gradients               rtol 1e-4, atol 1e-6 max|g| (test_loss_in_forward_gpu.py's: the per-triangle sums are
                                 float atomics)
  soup fuzz                      each route against the float64 truth within backward_fuzz's rounding bound (the rule
                                 fuzz_shade_backward_gpu.py applies to every lane variant)
The scenes are the cases of test_loss_in_forward_gpu.py: the shapes at which the forward kernel takes its other paths.

Largest deviation between the two routes' vertex gradients seen with the shipped form (the ordinary division, the
forward's own quotient), as a fraction of max|g|: 1.8e-7 (region kinds), 1.4e-8 (crowded block), 4.2e-8 - 8.4e-8 (extra
record slots), 1.8e-7 (32-pixel regions) -- _route_pair prints them under `pytest -s`.  The rebuilt barycentrics have
the stored ones' bits, so what remains is the order of the float atomics.  The soup fuzz read 0.005 of the float64
rounding bound on both routes."""
import contextlib

import numpy as np
import pytest
import torch

import backward_fuzz
from oracle import truth64
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import synthetic
from pytorch_mesh_renderer_amd.mesh_renderer import rasterize_triangles_ext as ext

pytestmark = pytest.mark.gpu
losses = mesh_renderer.losses
NO_BARY = "ShadeFoldLaneNoBaryFn"


@contextlib.contextmanager
def _region_edge(edge):
    assert _native.lib().mr_debug_set_raster_region_edge(edge) == 0
    try:
        yield
    finally:
        _native.lib().mr_debug_set_raster_region_edge(0)


@contextlib.contextmanager
def _remembered(target):
    losses.remember_target(target)
    try:
        yield target
    finally:
        losses.forget_target(target)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _on_device(job, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in job.items()}


def _random_target(shape, seed, device):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).to(device)


def _soup_job(n_tri, lo, hi, seed, device):
    """test_loss_in_forward_gpu.py's crowded block: n_tri small random triangles facing a camera at (0, 0, 3)."""
    g = torch.Generator().manual_seed(seed)
    centre = lo + (hi - lo) * torch.rand(n_tri, 1, 2, generator=g)
    xy = (centre + 0.06 * (torch.rand(n_tri, 3, 2, generator=g) - 0.5)).clamp(lo, hi)
    z = 0.04 * (torch.rand(n_tri, 1, 1, generator=g) - 0.5).expand(n_tri, 3, 1)
    verts = torch.cat([xy, z], dim=2).reshape(1, 3 * n_tri, 3).contiguous()
    tris = torch.arange(3 * n_tri, dtype=torch.int32).reshape(n_tri, 3)
    flip = torch.rand(n_tri, generator=g) < 0.5
    tris[flip] = tris[flip].flip(1)
    eyes = torch.tensor([[0.0, 0.0, 3.0]])
    job = {"vertices": verts, "triangles": tris.contiguous(),
           "normals": torch.tensor([0.0, 0.0, 1.0]).expand(1, 3 * n_tri, 3).contiguous(),
           "diffuse": torch.rand(1, 3 * n_tri, 3, generator=g), "eyes": eyes,
           "light_positions": eyes.unsqueeze(1).contiguous(), "light_intensities": torch.ones(1, 1, 3)}
    return _on_device(job, device)


def _same_grads(got, want, what=""):
    scale = float(want.abs().max())
    assert scale > 0
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-6 * scale, err_msg=what)
    return float((got - want).abs().max()) / scale


def _native_pair(d, w, h, target):
    """The loss-in-forward call with the private G-buffer against the same call without it."""
    xf = synthetic.clip_transforms(d["eyes"].cpu(), w, h).to(target.device)
    args = (d["vertices"], xf, d["normals"], d["diffuse"], d["triangles"], d["light_positions"], d["light_intensities"],
            None, w, h)
    kw = dict(want_z=False, want_empty_regions=True, prepare_backward=True, l1_target=target,
              l1_target_empty=_native.image_empty_regions(target))
    off = _native.render_forward(*args, **kw)
    on = _native.render_forward(*args, **kw, private_gbuffer=True)
    assert on[2] is None, "no barycentric tensor"
    assert torch.equal(_bits(on[4]), _bits(off[4])), "image"
    assert torch.equal(on[6], off[6]), "empty-region map"
    assert torch.equal(_bits(on[-1][0]), _bits(off[-1][0])), "loss"
    assert torch.equal(on[-1][1], off[-1][1]), "sign codes"
    covered = off[2].sum(-1) > 0.5
    assert torch.equal(on[1].clamp(min=0), off[1]), "ids after -1 -> 0"
    assert torch.equal(on[1] >= 0, covered), "-1 exactly where nothing was drawn"
    batch, n_tri = d["vertices"].shape[0], d["triangles"].shape[0]
    assert on[-2].numel() >= _native.lib().mr_render_forward_l1_private_bytes(batch, n_tri, w, h) \
        > _native.lib().mr_shade_backward_prepared_bytes(batch, n_tri)
    return off, on


def _step(d, w, h, target, private, after_loss=None, backwards=1):
    """render() + l1_loss + backward with the switch `private` -> (loss, vertex gradients, image, kernel name)."""
    v = d["vertices"].clone().requires_grad_(True)
    with ext.private_gbuffer(private):
        img = mesh_renderer.render(v, d["triangles"], d["normals"], d["diffuse"], d["eyes"], torch.zeros_like(d["eyes"]),
                                   torch.tensor([0.0, 1.0, 0.0], device=v.device), d["light_positions"],
                                   d["light_intensities"], w, h)
    assert img.grad_fn.prepared_state["private"] is bool(private)
    loss = losses.l1_loss(img, target)
    assert loss.grad_fn.loss_from_forward is True
    seen = after_loss(img) if after_loss is not None else None
    grads, kernels = [], []
    for k in range(backwards):
        v.grad = None
        loss.backward(retain_graph=k + 1 < backwards)
        kernels.append(_native.debug_last_accumulate_kernel())
        grads.append(v.grad.clone())
    return loss.detach(), grads, img.detach(), kernels, seen


def _route_pair(d, w, h, target):
    with _remembered(target):
        l_on, (g_on,), img_on, (k_on,), _ = _step(d, w, h, target, True)
        l_off, (g_off,), img_off, (k_off,), _ = _step(d, w, h, target, False)
    assert NO_BARY in k_on and NO_BARY not in k_off and "ShadeFoldLaneFn<1, true>" in k_off, (k_on, k_off)
    assert torch.equal(_bits(img_on), _bits(img_off))
    assert torch.equal(_bits(l_on), _bits(l_off))
    worst = _same_grads(g_on, g_off)
    print("largest |g_on - g_off| / max|g| = %.3e" % worst)
    return g_off


def test_region_kinds(device):
    """200 x 136, batch 2, a 0.45-scaled sphere at 64-pixel regions: empty, both-empty, ragged and ordinary regions."""
    w, h, batch = 200, 136, 2
    job = synthetic.sphere_job(batch, w, h, 12)
    job["vertices"] = (job["vertices"] * 0.45).contiguous()
    d = _on_device(job, device)
    target = torch.zeros(batch, h, w, 4)
    rnd = torch.rand(batch, h, w, 4, generator=torch.Generator().manual_seed(3))
    target[:, :, 64:] = rnd[:, :, 64:]
    target[:, :8, :64] = rnd[:, :8, :64]
    target[:, 90:120, 10:50] = rnd[:, 90:120, 10:50]
    target = target.to(device).contiguous()
    with _region_edge(64):
        off, _ = _native_pair(d, w, h, target)
        rmap = off[6]
        assert int(rmap[0, 0, 0]) == 1 and int(rmap[0, 1, 0]) == 1 and int(rmap[0, 0, 1]) == 0
        _route_pair(d, w, h, target)


def test_crowded_region_takes_several_bin_rounds(device):
    """300 small triangles inside one 64 x 64 block of 256 x 256: several bin rounds (a later round rebuilds the pixel
    state an earlier one left, barycentrics included) and the scalar record path."""
    w = h = 256
    d = _soup_job(300, -0.50, -0.08, 11, device)
    target = _random_target((1, h, w, 4), 5, device)
    with _region_edge(64):
        off, _ = _native_pair(d, w, h, target)
        assert int(off[1][0][off[2][0].sum(-1) > 0.5].unique().numel()) >= 40
        _route_pair(d, w, h, target)


def test_extra_record_slots_instantiation(device):
    """128 x 128 with the resolution-12 sphere at 64-pixel regions: the instantiation with extra record slots."""
    w = h = 128
    job = synthetic.sphere_job(1, w, h, 12)
    assert job["triangles"].shape[0] * 4096 >= 32 * w * h
    d = _on_device(job, device)
    target = _random_target((1, h, w, 4), 6, device)
    target[:, :, :32] = 0.0
    with _region_edge(64):
        _native_pair(d, w, h, target)
        _route_pair(d, w, h, target)


def test_32_pixel_regions(device):
    """96 x 80, batch 2: the automatic choice is 32-pixel regions, ragged at the top."""
    w, h, batch = 96, 80, 2
    assert _native.lib().mr_render_forward_l1_partials(batch, w, h) == batch * 3 * 3
    d = _on_device(synthetic.sphere_job(batch, w, h, 8), device)
    target = _random_target((batch, h, w, 4), 7, device)
    target[:, 16:, :64] = 0.0
    _native_pair(d, w, h, target)
    _route_pair(d, w, h, target)


@pytest.fixture(scope="module")
def small_scene(device):
    w, h, batch = 200, 136, 2
    d = _on_device(synthetic.sphere_job(batch, w, h, 12), device)
    target = _random_target((batch, h, w, 4), 21, device)
    with _remembered(target):
        loss, (grad,), _, _, _ = _step(d, w, h, target, False)     # the switch-off route, computed once
    return d, w, h, target, loss, grad


_UP = {}


def _render(d, w, h, leaves):
    device = d["eyes"].device     # (the up vector is uploaded once: a host-to-device copy cannot be captured)
    if device not in _UP:
        _UP[device] = torch.tensor([0.0, 1.0, 0.0], device=device)
    up = _UP[device]
    return mesh_renderer.render(leaves["vertices"], d["triangles"], leaves["normals"], leaves["diffuse"], d["eyes"],
                                torch.zeros_like(d["eyes"]), up, d["light_positions"], d["light_intensities"], w, h)


def test_mode_is_declined(device, small_scene):
    """Normals or diffuse colours that require grad, no remembered target, more than four lights, the switch off."""
    d, w, h, target, _, _ = small_scene
    plain = {k: d[k].clone() for k in ("vertices", "normals", "diffuse")}
    with _remembered(target):
        for also in ("normals", "diffuse"):
            leaves = dict(plain, vertices=plain["vertices"].clone().requires_grad_(True), **{also: plain[also].clone().requires_grad_(True)})
            img = _render(d, w, h, leaves)
            assert img.grad_fn.l1_in_forward is not None and img.grad_fn.prepared_state["private"] is False
            losses.l1_loss(img, target).backward()
            assert NO_BARY not in _native.debug_last_accumulate_kernel()
        leaves = dict(plain, vertices=plain["vertices"].clone().requires_grad_(True))
        with ext.private_gbuffer(False):
            assert _render(d, w, h, leaves).grad_fn.prepared_state["private"] is False
        assert _render(d, w, h, leaves).grad_fn.prepared_state["private"] is True
        five = dict(d, light_positions=d["light_positions"].expand(-1, 5, -1).contiguous(),
                    light_intensities=(d["light_intensities"].expand(-1, 5, -1) * 0.2).contiguous())
        assert _render(five, w, h, leaves).grad_fn.prepared_state["private"] is False
    leaves = dict(plain, vertices=plain["vertices"].clone().requires_grad_(True))
    img = _render(d, w, h, leaves)
    assert img.grad_fn.l1_in_forward is None and img.grad_fn.prepared_state["private"] is False


def test_slow_paths_get_the_public_gbuffer(device, small_scene):
    """Consumers the private G-buffer cannot serve get the switch-off route's values: a second backward over a retained
    graph, retain_grad() on the image, a hook registered after the loss, autograd.grad naming the image."""
    d, w, h, target, l_ref, g_ref = small_scene
    with _remembered(target):
        _, (g,), _, _, img = _step(d, w, h, target, False, after_loss=lambda img: (img.retain_grad(), img)[1])
        dimage_ref = img.grad.clone()      # the switch-off route's dense image gradient
        _same_grads(g, g_ref)
        assert float(dimage_ref.abs().max()) > 0
        # two backwards: the first on the private G-buffer, the second on the public one
        loss, grads, _, kernels, _ = _step(d, w, h, target, True, backwards=2)
        assert torch.equal(_bits(loss), _bits(l_ref))
        assert NO_BARY in kernels[0] and NO_BARY not in kernels[1], kernels
        for g in grads:
            _same_grads(g, g_ref)
        # retain_grad(): the image's dense gradient is formed and the renderer's node carries it on
        loss, (g,), _, (k,), img = _step(d, w, h, target, True, after_loss=lambda img: (img.retain_grad(), img)[1])
        assert NO_BARY not in k
        _same_grads(g, g_ref)
        assert torch.equal(img.grad, dimage_ref)
        # a hook registered after the loss was built
        seen = []
        loss, (g,), _, (k,), _ = _step(d, w, h, target, True, after_loss=lambda img: img.register_hook(lambda gr: seen.append(gr.clone())))
        assert NO_BARY not in k and len(seen) == 1 and torch.equal(seen[0], dimage_ref)
        _same_grads(g, g_ref)
        # autograd.grad naming the image
        v = d["vertices"].clone().requires_grad_(True)
        img = _render(d, w, h, dict(d, vertices=v))
        assert img.grad_fn.prepared_state["private"] is True
        loss = losses.l1_loss(img, target)
        dimg, dv = torch.autograd.grad(loss, [img, v])
        assert NO_BARY not in _native.debug_last_accumulate_kernel()
        assert torch.equal(dimg, dimage_ref)
        _same_grads(dv, g_ref)


def test_modes_switched_on_between_forward_and_backward(device, small_scene):
    """The deterministic mode, or the rows kernel forced, AFTER render() has written the private G-buffer: the kernel that
    reads it does not run in either, so the backward takes the public G-buffer and the mode's own kernels."""
    d, w, h, target, l_ref, g_ref = small_scene
    with _remembered(target):
        for switch, on, off in ((_native.set_deterministic, True, False), (_native.debug_set_shade_backward_kernel, 1, 0)):
            v = d["vertices"].clone().requires_grad_(True)
            img = _render(d, w, h, dict(d, vertices=v))
            assert img.grad_fn.prepared_state["private"] is True
            loss = losses.l1_loss(img, target)
            switch(on)
            try:
                loss.backward()
            finally:
                switch(off)
            assert NO_BARY not in _native.debug_last_accumulate_kernel()
            assert torch.equal(_bits(loss.detach()), _bits(l_ref))
            _same_grads(v.grad, g_ref)


def test_soup_fuzz_against_the_float64_truth(device):
    """200 random soups at 64 x 64 (slivers, one-pixel triangles, both windings): the private route's and the public
    route's vertex gradients, each against the float64 truth on the stored barycentrics within backward_fuzz's
    rounding bound."""
    rng = np.random.default_rng(20240)
    report = backward_fuzz.Report()
    W = H = 64
    up = torch.full((1,), 0.9, device=device)
    with_gradients = 0
    for trial in range(200):
        B, V, T, _, _, pos, xf, tris = backward_fuzz.soup(rng, trial, True)
        L = int(rng.integers(1, 5))
        nrm = rng.normal(size=(B, V, 3)).astype(np.float32)
        kd = rng.random(size=(B, V, 3)).astype(np.float32)
        lp = (rng.normal(size=(B, L, 3)) * 3.0).astype(np.float32)
        li = (rng.random(size=(B, L, 3)) + 0.1).astype(np.float32)
        amb = (rng.random(size=(B, 3)) * 0.3).astype(np.float32) if trial % 3 == 0 else None
        target = torch.from_numpy(rng.random(size=(B, H, W, 4)).astype(np.float32)).to(device)
        pos_d, xf_d, tris_d, nrm_d, kd_d, lp_d, li_d, amb_d = map(backward_fuzz._dev, (pos, xf, tris, nrm, kd, lp, li, amb))
        fwd = (pos_d, xf_d, nrm_d, kd_d, tris_d, lp_d, li_d, amb_d, W, H)
        clip, ids, bary, _, rgba, _ = _native.render_forward(*fwd, want_z=False)
        ids_h, bary_h = ids.cpu().numpy(), bary.cpu().numpy()
        mask = torch.from_numpy(truth64.borderline_pixels(ids_h, bary_h, tris, nrm, pos, kd, lp, li, amb)).to(device)
        target[mask] = rgba[mask]            # sign 0 at the borderline pixels, as backward_fuzz._switch_off does
        sign_g = (torch.sign(rgba - target) * (0.9 / rgba.numel())).cpu().numpy()
        t = truth64.phong(ids_h, bary_h, tris, nrm, pos, kd, lp, li, amb, sign_g)
        d_clip, noise_clip = truth64.raster_pullback(clip.cpu().numpy(), tris, ids_h, bary_h, t["dbary"], t["gabs"])
        truth, noise = truth64.whole_vertex_gradient(xf, t["d_positions"], d_clip, t["noise_positions"], noise_clip)
        with_gradients += int(float(np.abs(truth).max()) > 0)
        adjacency = _native.vertex_adjacency(tris_d, V)
        for private in (True, False):
            out = _native.render_forward(*fwd, want_z=False, prepare_backward=True, l1_target=target, private_gbuffer=private)
            assert torch.equal(_bits(out[4]), _bits(rgba))
            grads = _native.shade_backward(up, out[1], out[2], out[0], nrm_d, pos_d, kd_d, tris_d, lp_d, li_d, amb_d,
                                           corner_records=out[5], adjacency=adjacency, l1_signs=out[-1][1], transforms=xf_d,
                                           want_light_grads=False, want_normal_grads=False, want_diffuse_grads=False,
                                           want_clip_grads=False, normalised_gbuffer=True, prepared=out[-2],
                                           private_gbuffer=private)
            kernel = _native.debug_last_accumulate_kernel()
            assert (NO_BARY in kernel) is private, kernel
            report.check("private" if private else "public", "d vertices", grads[2], truth, noise,
                         "trial %d B=%d V=%d T=%d L=%d" % (trial, B, V, T, L))
    print("worst excess (error / bound):", report.summary())
    assert not report.failures, report.failures[:10]
    assert with_gradients >= 100


def test_captured_step(device):
    """capture_step over the private route, replayed twice with eager work in between: loss and gradients equal the
    eager switch-off step's."""
    w = h = 96
    d = _on_device(synthetic.sphere_job(2, w, h, 8), device)
    vertices = d["vertices"].clone().requires_grad_(True)
    with torch.no_grad():
        target = _render(d, w, h, d).roll(4, 2).contiguous()
    kernels = []

    def step():
        img = _render(d, w, h, dict(d, vertices=vertices))
        assert img.grad_fn.prepared_state["private"] is True
        loss = losses.l1_loss(img, target)
        loss.backward()
        kernels.append(_native.debug_last_accumulate_kernel())
        return loss
    with _remembered(target):
        l_ref, (g_ref,), _, _, _ = _step(d, w, h, target, False)
        captured = mesh_renderer.capture_step(step, [vertices])
        assert kernels and all(NO_BARY in k for k in kernels)
        for _ in range(2):
            loss = captured.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(loss.detach()), _bits(l_ref))
            _same_grads(vertices.grad, g_ref)
            _, (g_eager,), _, _, _ = _step(d, w, h, target, True)     # eager work between the replays
            _same_grads(g_eager, g_ref)
