"""mean|image - target| computed by the fused forward's epilogue for a remembered target (mr_render_forward_l1,
rasterize_triangles_ext.loss_in_forward).  The yardstick everywhere is the stand-alone route on the same scene: the
plain forward followed by _native.l1_loss_forward(image, target), and render() + l1_loss with the switch off.
  sign codes                 torch.equal
  image, ids, barycentrics   torch.equal (bit patterns) with the switch off
  loss                       1e-6 relative (the bound between the loss's two groupings of its sum in
                             test_render_empty_block_map_serves_the_loss_and_the_backward)
  vertex gradients           rtol 1e-4, atol 1e-6 max|g| (that test's; the per-triangle sums are float atomics)"""
import contextlib
import math

import numpy as np
import pytest
import torch

from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import synthetic
from pytorch_mesh_renderer_amd.mesh_renderer import rasterize_triangles_ext as ext

pytestmark = pytest.mark.gpu
losses = mesh_renderer.losses


@contextlib.contextmanager
def _region_edge(edge):
    assert _native.lib().mr_debug_set_raster_region_edge(edge) == 0
    try:
        yield
    finally:
        _native.lib().mr_debug_set_raster_region_edge(0)


@contextlib.contextmanager
def _spy_render_forward():
    """Records, per call of _native.render_forward, whether it was handed a loss target."""
    seen, real = [], _native.render_forward

    def spy(*args, **kwargs):
        seen.append(kwargs.get("l1_target") is not None)
        return real(*args, **kwargs)
    _native.render_forward = spy
    try:
        yield seen
    finally:
        _native.render_forward = real


def _bits(t):
    return t.contiguous().view(torch.int32)


def _on_device(job, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in job.items()}


def _same_loss(got, want):
    got, want = float(got), float(want)
    if math.isfinite(want):
        assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    else:
        assert (math.isnan(got) and math.isnan(want)) or got == want, (got, want)


def _native_pair(d, w, h, target, target_map=None):
    """The plain forward and the forward with the loss on the same inputs -> (plain outputs, rendered empty map, loss,
    signs); asserts the G-buffer and the image bit for bit, the codes and the loss against the stand-alone kernel."""
    xf = synthetic.clip_transforms(d["eyes"].cpu(), w, h).to(target.device)
    args = (d["vertices"], xf, d["normals"], d["diffuse"], d["triangles"], d["light_positions"], d["light_intensities"],
            None, w, h)
    plain = _native.render_forward(*args, want_z=False, want_empty_regions=True)
    fused = _native.render_forward(*args, want_z=False, want_empty_regions=True, l1_target=target,
                                   l1_target_empty=target_map)
    loss, signs = fused[-1]
    for i, name in ((1, "ids"), (2, "bary"), (4, "rgba")):
        assert torch.equal(_bits(fused[i]), _bits(plain[i])), name
    assert torch.equal(fused[6], plain[6]), "the renderer's own empty-block map"
    want_loss, want_signs = _native.l1_loss_forward(plain[4], target, want_signs=True)
    assert signs.shape == want_signs.shape and torch.equal(signs, want_signs), "sign codes"
    _same_loss(loss, want_loss)
    return plain, plain[6], loss, signs


def _step(d, w, h, target, on, spelled=False, backwards=1):
    """render() + L1 loss + backward with the switch `on` -> (loss, vertex gradient, image, loss node's flag)."""
    v = d["vertices"].clone().requires_grad_(True)
    with ext.loss_in_forward(on):
        img = mesh_renderer.render(v, d["triangles"], d["normals"], d["diffuse"], d["eyes"], torch.zeros_like(d["eyes"]),
                                   torch.tensor([0.0, 1.0, 0.0], device=v.device), d["light_positions"],
                                   d["light_intensities"], w, h)
        loss = torch.mean(torch.abs(img - target)) if spelled else losses.l1_loss(img, target)
    grads = []
    for k in range(backwards):
        v.grad = None
        loss.backward(retain_graph=k + 1 < backwards)
        grads.append(v.grad.clone())
    return loss.detach(), grads if backwards > 1 else grads[0], img.detach(), loss.grad_fn.loss_from_forward


def _same_grads(got, want, what=""):
    scale = float(want.abs().max())
    assert scale > 0
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-6 * scale, err_msg=what)


def _route_pair(d, w, h, target, **kwargs):
    """The step with the switch on (must take the new route) against the step with it off."""
    l_on, g_on, img_on, flag_on = _step(d, w, h, target, True, **kwargs)
    l_off, g_off, img_off, flag_off = _step(d, w, h, target, False, **kwargs)
    assert flag_on is True and flag_off is False
    assert torch.equal(_bits(img_on), _bits(img_off))
    _same_loss(l_on, l_off)
    _same_grads(g_on, g_off)
    return l_on


def _soup_job(n_tri, lo, hi, seed, device):
    """n_tri small random triangles facing a camera at (0, 0, 3): world (x, y) in [lo, hi]^2 lands at
    pixel = (x / (3 tan 20 deg) + 1) / 2 * size of a square image."""
    g = torch.Generator().manual_seed(seed)
    centre = lo + (hi - lo) * torch.rand(n_tri, 1, 2, generator=g)
    xy = centre + 0.06 * (torch.rand(n_tri, 3, 2, generator=g) - 0.5)
    xy = xy.clamp(lo, hi)
    z = 0.04 * (torch.rand(n_tri, 1, 1, generator=g) - 0.5).expand(n_tri, 3, 1)
    verts = torch.cat([xy, z], dim=2).reshape(1, 3 * n_tri, 3).contiguous()
    tris = torch.arange(3 * n_tri, dtype=torch.int32).reshape(n_tri, 3)
    flip = torch.rand(n_tri, generator=g) < 0.5           # both windings
    tris[flip] = tris[flip].flip(1)
    eyes = torch.tensor([[0.0, 0.0, 3.0]])
    job = {"vertices": verts, "triangles": tris.contiguous(),
           "normals": torch.tensor([0.0, 0.0, 1.0]).expand(1, 3 * n_tri, 3).contiguous(),
           "diffuse": torch.rand(1, 3 * n_tri, 3, generator=g), "eyes": eyes,
           "light_positions": eyes.unsqueeze(1).contiguous(), "light_intensities": torch.ones(1, 1, 3)}
    return _on_device(job, device)


def _random_target(shape, seed, device):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).to(device)


def test_region_kinds(device):
    """Case 1.  64-pixel regions on a 200 x 136 image (neither a multiple of 64), a small sphere in the middle: regions
    the render leaves empty whose target holds content, regions empty on both sides, ragged regions at the right and
    top edges and ordinary ones -- each kind asserted to occur."""
    w, h, batch = 200, 136, 2
    job = synthetic.sphere_job(batch, w, h, 12)
    job["vertices"] = (job["vertices"] * 0.45).contiguous()
    d = _on_device(job, device)
    target = torch.zeros(batch, h, w, 4)
    rnd = torch.rand(batch, h, w, 4, generator=torch.Generator().manual_seed(3))
    target[:, :, 64:] = rnd[:, :, 64:]            # every block column but the first, the ragged one included
    target[:, :8, :64] = rnd[:, :8, :64]          # the ragged top band of the first column (G-buffer rows 128..135)
    target[:, 90:120, 10:50] = rnd[:, 90:120, 10:50]   # inside block (0, 0): G-buffer rows 0..63 are image rows 72..135
    target = target.to(device).contiguous()           # block (1, 0), image rows 8..71, stays zero
    with _region_edge(64):
        assert _native.lib().mr_render_forward_l1_partials(batch, w, h) == batch * 4 * 3
        tmap = _native.image_empty_regions(target)
        for use_map in (tmap, None):
            plain, rmap, _, _ = _native_pair(d, w, h, target, use_map)
        assert rmap.shape == (batch, 3, 4)
        alpha = plain[4][..., 3]
        for b in range(batch):
            assert int(rmap[b, 0, 0]) == 1 and int(tmap[b, 0, 0]) == 0, "empty region, target with content"
            assert int(rmap[b, 1, 0]) == 1 and int(tmap[b, 1, 0]) == 1, "empty on both sides"
            assert int(rmap[b, 2, 1]) == 0 and int(rmap[b, 1, 3]) == 0, "ragged regions are never marked"
            assert float(target[b, :8].abs().sum()) > 0 and float(target[b, :, 192:].abs().sum()) > 0
            # an ordinary region: whole, with covered and uncovered pixels (block (0, 1): image rows 72..135, columns 64..127)
            cover = float(alpha[b, 72:136, 64:128].mean())
            assert int(rmap[b, 0, 1]) == 0 and 0.05 < cover < 0.95, cover
        losses.remember_target(target)
        try:
            _route_pair(d, w, h, target)
        finally:
            losses.forget_target(target)


def test_crowded_region_takes_several_bin_rounds(device):
    """Case 2.  300 small triangles inside ONE 64 x 64 block of a 256 x 256 image: more candidates than the bin's 256
    entries (several bin rounds, the epilogue on the last one only, corner records one winner at a time through the
    scalar cache), below the density that selects the instantiation with extra record slots."""
    w = h = 256
    n_tri = 300
    assert n_tri > 256 and n_tri * 4096 < 32 * w * h
    d = _soup_job(n_tri, -0.50, -0.08, 11, device)
    target = _random_target((1, h, w, 4), 5, device)
    with _region_edge(64):
        plain, _, _, _ = _native_pair(d, w, h, target, _native.image_empty_regions(target))
        covered = (plain[2].sum(-1) > 0.5)[0].nonzero()
        assert covered.shape[0] > 300
        rows, cols = covered[:, 0], covered[:, 1]
        assert int(rows.min()) // 64 == int(rows.max()) // 64 and int(cols.min()) // 64 == int(cols.max()) // 64, \
            "all triangles inside one block"
        assert int(plain[1][0][plain[2][0].sum(-1) > 0.5].unique().numel()) >= 40
        losses.remember_target(target)
        try:
            _route_pair(d, w, h, target)
        finally:
            losses.forget_target(target)


def test_extra_record_slots_instantiation(device):
    """Case 3.  128 x 128 with at least 128 triangles at 64-pixel regions: the density rule selects the instantiation
    with extra record slots."""
    w = h = 128
    job = synthetic.sphere_job(1, w, h, 12)
    assert job["triangles"].shape[0] * 4096 >= 32 * w * h
    d = _on_device(job, device)
    target = _random_target((1, h, w, 4), 6, device)
    target[:, :, :32] = 0.0
    with _region_edge(64):
        _native_pair(d, w, h, target, _native.image_empty_regions(target))
        losses.remember_target(target)
        try:
            _route_pair(d, w, h, target)
        finally:
            losses.forget_target(target)


def test_32_pixel_regions(device):
    """Case 4.  A small launch with the region edge left automatic runs 32-pixel regions (96 x 80: ragged at the top);
    the target's 64-pixel block map is then not consulted."""
    w, h, batch = 96, 80, 2
    assert _native.lib().mr_render_forward_l1_partials(batch, w, h) == batch * 3 * 3
    d = _on_device(synthetic.sphere_job(batch, w, h, 8), device)
    target = _random_target((batch, h, w, 4), 7, device)
    target[:, 16:, :64] = 0.0                         # block (0, 0) of the target's map is whole and empty
    tmap = _native.image_empty_regions(target)
    assert int(tmap[0, 0, 0]) == 1
    _native_pair(d, w, h, target, tmap)
    losses.remember_target(target)
    try:
        _route_pair(d, w, h, target)
    finally:
        losses.forget_target(target)


def test_odd_target_values(device):
    """Case 5.  Target pixels equal to the render's own, +0, -0, NaN and +-inf: the codes equal the stand-alone
    kernel's everywhere (asserted inside _native_pair), and the loss is the same NaN / infinity / number."""
    w, h, batch = 200, 136, 2
    job = synthetic.sphere_job(batch, w, h, 12)
    job["vertices"] = (job["vertices"] * 0.45).contiguous()
    d = _on_device(job, device)
    xf = synthetic.clip_transforms(job["eyes"], w, h).to(device)
    with _region_edge(64):
        own = _native.render_forward(d["vertices"], xf, d["normals"], d["diffuse"], d["triangles"], d["light_positions"],
                                     d["light_intensities"], None, w, h, want_z=False)[4]
        target = own.clone()                                  # d = 0 on every pixel ...
        g = torch.Generator().manual_seed(9)
        finite = target.clone()
        pick = torch.rand(batch, h, w, 4, generator=g).to(device)
        finite[pick < 0.05] = -0.0
        finite[(pick >= 0.05) & (pick < 0.10)] = 0.0
        finite[(pick >= 0.10) & (pick < 0.15)] = 0.25
        _, _, loss, signs = _native_pair(d, w, h, finite.contiguous(), _native.image_empty_regions(finite))
        assert math.isfinite(float(loss)) and float(loss) > 0 and int((signs == 0).sum()) > 0
        for value in (float("nan"), float("inf"), float("-inf")):
            odd = finite.clone()
            odd[(pick >= 0.20) & (pick < 0.22)] = value
            odd[0, 100, 20, 1] = value                         # inside a block the render leaves empty
            odd[1, 3, 196, 2] = value                          # inside the ragged corner region
            for tmap in (_native.image_empty_regions(odd), None):
                _, _, loss, _ = _native_pair(d, w, h, odd.contiguous(), tmap)
                assert not math.isfinite(float(loss))


@pytest.fixture(scope="module")
def small_scene(device):
    w, h, batch = 200, 136, 2
    job = synthetic.sphere_job(batch, w, h, 12)
    d = _on_device(job, device)
    targets = [_random_target((batch, h, w, 4), seed, device) for seed in (21, 22)]
    reference = [_step(d, w, h, t, False)[:2] for t in targets]     # the stand-alone route, computed once
    return d, w, h, targets, reference


def test_fallbacks(device, small_scene):
    """Case 6.  Every case that does not match exactly runs the stand-alone loss kernel -- and is right; the loss
    node's loss_from_forward tells which route it took."""
    d, w, h, (t1, t2), ((l1_ref, g1_ref), (l2_ref, g2_ref)) = small_scene
    losses.remember_target(t1)
    losses.remember_target(t2)
    try:
        # two remembered targets of one shape: the newer is served by the forward, the older by the loss kernel
        for target, l_ref, g_ref, from_forward in ((t2, l2_ref, g2_ref, True), (t1, l1_ref, g1_ref, False)):
            with _spy_render_forward() as seen:
                loss, grad, _, flag = _step(d, w, h, target, True)
            assert seen == [True] and flag is from_forward
            _same_loss(loss, l_ref)
            _same_grads(grad, g_ref)
        # the reference's spelling takes the new route too
        loss, grad, _, flag = _step(d, w, h, t2, True, spelled=True)
        assert flag is True
        _same_loss(loss, l2_ref)
        _same_grads(grad, g2_ref)
        # two backwards over a retained graph
        loss, grads, _, flag = _step(d, w, h, t2, True, backwards=2)
        assert flag is True
        for g in grads:
            _same_grads(g, g2_ref)
        # render() under no_grad: nothing to differentiate, no target read
        with _spy_render_forward() as seen, torch.no_grad():
            img = mesh_renderer.render(d["vertices"], d["triangles"], d["normals"], d["diffuse"], d["eyes"],
                                       torch.zeros_like(d["eyes"]), torch.tensor([0.0, 1.0, 0.0], device=device),
                                       d["light_positions"], d["light_intensities"], w, h)
        assert seen == [False] and img.grad_fn is None
        # the target edited in place between render() and the loss: the forward's numbers are stale and not used
        edited = t2.clone()
        losses.remember_target(edited)
        v = d["vertices"].clone().requires_grad_(True)
        img = mesh_renderer.render(v, d["triangles"], d["normals"], d["diffuse"], d["eyes"], torch.zeros_like(d["eyes"]),
                                   torch.tensor([0.0, 1.0, 0.0], device=device), d["light_positions"],
                                   d["light_intensities"], w, h)
        assert img.grad_fn.l1_in_forward is not None
        edited.copy_(t1)
        loss = losses.l1_loss(img, edited)
        assert loss.grad_fn.loss_from_forward is False
        loss.backward()
        _same_loss(loss.detach(), l1_ref)
        _same_grads(v.grad, g1_ref)
        # ... and the next render() does not take the route for it either, until it is remembered again
        with _spy_render_forward() as seen:
            _, _, _, flag = _step(d, w, h, edited, True)
        assert seen == [False] and flag is False
        losses.remember_target(edited)
        loss, grad, _, flag = _step(d, w, h, edited, True)
        assert flag is True
        _same_loss(loss, l1_ref)
        _same_grads(grad, g1_ref)
        # the image edited in place (under no_grad it keeps its node): the loss reads it back
        v = d["vertices"].clone().requires_grad_(True)
        img = mesh_renderer.render(v, d["triangles"], d["normals"], d["diffuse"], d["eyes"], torch.zeros_like(d["eyes"]),
                                   torch.tensor([0.0, 1.0, 0.0], device=device), d["light_positions"],
                                   d["light_intensities"], w, h)
        with torch.no_grad():
            img[..., 3] = 1.0
        loss = losses.l1_loss(img, edited)
        assert loss.grad_fn.loss_from_forward is False
        _same_loss(loss.detach(), torch.mean(torch.abs(img.detach() - edited)))
        # forget_target: the renderer no longer knows of it
        losses.forget_target(edited)
        with _spy_render_forward() as seen:
            loss, grad, _, flag = _step(d, w, h, edited, True)
        assert seen == [False] and flag is False
        _same_loss(loss, l1_ref)
        _same_grads(grad, g1_ref)
    finally:
        for t in (t1, t2):
            losses.forget_target(t)


def test_captured_step_follows_the_target(device):
    """Case 7.  The route under stream capture: a replay equals the eager stand-alone step; after target.copy_(new) and
    remember_target(target) -- which refreshes the target's map in place -- the same graph serves the new target."""
    w = h = 96
    d = _on_device(synthetic.sphere_job(2, w, h, 8), device)
    vertices = d["vertices"].clone().requires_grad_(True)
    center, up = torch.zeros_like(d["eyes"]), torch.tensor([0.0, 1.0, 0.0], device=device)

    def render():
        return mesh_renderer.render(vertices, d["triangles"], d["normals"], d["diffuse"], d["eyes"], center, up,
                                    d["light_positions"], d["light_intensities"], w, h)
    with torch.no_grad():
        first = render().roll(4, 2).contiguous()
        second = render().roll(-9, 1).contiguous()
        second[:, :, :40] = 0.0
    target = losses.remember_target(first.clone())
    kept_map = ext._target_empty_regions(target)
    routes = []

    def step():
        loss = losses.l1_loss(render(), target)
        routes.append(loss.grad_fn.loss_from_forward)
        loss.backward()
        return loss

    def eager_reference():
        keep, vertices.grad = vertices.grad, None
        with ext.loss_in_forward(False):
            loss = float(step().detach())
        grad, vertices.grad = vertices.grad, keep
        return loss, grad
    try:
        captured = mesh_renderer.capture_step(step, [vertices])
        assert routes and all(routes)
        seen = []
        for new_target in (None, second):
            if new_target is not None:
                target.copy_(new_target)
                assert ext._target_empty_regions(target) is None
                losses.remember_target(target)
                assert ext._target_empty_regions(target) is kept_map, "the map is refreshed in place"
            loss = captured.replay()
            torch.cuda.synchronize()
            got_loss, got_grad = float(loss), vertices.grad.clone()
            want_loss, want_grad = eager_reference()
            assert routes[-1] is False
            _same_loss(got_loss, want_loss)
            _same_grads(got_grad, want_grad)
            seen.append(got_loss)
        assert abs(seen[1] - seen[0]) > 1e-3 * seen[0], "the replay did not see the new target"
    finally:
        losses.forget_target(target)


def test_pending_loss_timer_is_closed_as_an_empty_interval(device, small_scene):
    """A hipEvent pair armed for the loss kernel (bench.py's roofline_l1_forward) in a step whose loss comes out of the
    forward: both events are recorded, back to back, so the pair reads (nearly) zero -- it neither stays pending for some
    later loss kernel nor is left unrecorded (hipEventElapsedTime would fail and leave its error behind)."""
    import ctypes
    d, w, h, (t1, _), ((l_ref, _), _) = small_scene
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipEventCreate(ctypes.byref(a)) == 0 and hip.hipEventCreate(ctypes.byref(b)) == 0
    losses.remember_target(t1)
    try:
        _native.time_next_kernel(_native.TIMER_L1_FORWARD, a, b)
        loss, _, _, flag = _step(d, w, h, t1, True)
        assert flag is True and _native.TIMER_L1_FORWARD not in _native._pending_timers
        torch.cuda.synchronize()
        ms = ctypes.c_float(-1.0)
        assert hip.hipEventElapsedTime(ctypes.byref(ms), a, b) == 0
        assert 0.0 <= ms.value < 0.05, ms.value      # nothing in between: an empty pair is ~5 us of stream time, ten times that allowed
        _same_loss(loss, l_ref)
        # the next stand-alone loss is not bracketed by that pair: the slot is clear
        _, _, _, flag = _step(d, w, h, t1, False)
        assert flag is False
        ms2 = ctypes.c_float(-1.0)
        assert hip.hipEventElapsedTime(ctypes.byref(ms2), a, b) == 0 and ms2.value == ms.value
    finally:
        losses.forget_target(t1)
        hip.hipEventDestroy(a)
        hip.hipEventDestroy(b)
