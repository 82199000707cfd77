"""Camera gradients end to end -- render() and rasterize() differentiated to eye, center and up -- against a float64 truth.

Between the shading backward's d clip (held to the truth at the kernel boundary by tests/backward_fuzz.py) and the
gradient a camera receives lie the pull-back d clip -> d transforms (a torch matmul in FusedPhongRenderer._input_grads,
torch's own baddbmm backward on the specular and rasterize() routes) and the hand-derived camera backward
(k_camera_transforms_backward).  Here the truth is built from the G-buffer the forward wrote
(truth_helpers.scene_truth: truth64.phong -> raster_pullback), then

    d_xf[b,r,k] = sum_v d_clip[b,v,r] (v, 1)[k]        d_(eye, center, up) = J^T d_xf

with J the float64 Jacobian of tests/camera_reference.py (truth_helpers.camera_chain_truth, which also states the noise
scale), plus truth64.phong's d_camera for the eye of a specular render.  Everything is asserted with
truth64.assert_within_rounding (k_rounding = 64, floor 1e-7), borderline pixels switched off as backward_fuzz does.

Scenes (truth_helpers.camera_scene): the cube and an 8-ring sphere at 64 x 48, one backward_fuzz soup; two images, a
different plain-family camera per image (eye, center, up, fov, near, far all per image), 5 to 95 % of the pixels covered.

Every case checks d eye, d center, d up; with the vertices requiring grad also d vertices, which must hold the pulled-back
clip term although d clip is then emitted on its own; with everything requiring grad also d normals and d diffuse.

MEASURED on the MI355X, largest excess over the rounding bound (1 = at the bound) over all cases: d eye 8.5e-5, d center
9.7e-5, d up 8.5e-5, d vertices 2.4e-3, d normals 1.2e-2, d diffuse 2.4e-2 -- the same on every loss route and in
deterministic mode to within a factor of two.  Each case also prints the REACH of its bound, the excess a gradient of
zeros would have: 4 .. 6 (sphere), 14 .. 120 (cube), 84 .. 280 (soup) for the cameras, 1e3 .. 6e3 for d vertices.  The
camera bound is wide -- a camera's gradient is a sum over all vertices of clip-space terms that largely cancel, and the
noise scale adds their magnitudes -- so these cases see a lost, transposed or mis-signed term, not a last-digit error
(that is tests/test_camera_truth_gpu.py's part); every case asserts reach > 1.  Mutations (not committed): dxf
transposed fails 39 cases here at 9 .. 139 times the bound; the clip pull-back left out of d vertices when d clip is
emitted on its own fails 27 at 1200 .. 5700; two one-line mutations of k_camera_transforms_backward fail all 63 at
7 .. 2000.
"""
import functools

import numpy as np
import pytest
import torch

import camera_reference as cr
import truth_helpers as th
from oracle import truth64
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import camera_utils
from pytorch_mesh_renderer_amd.mesh_renderer import losses

pytestmark = pytest.mark.gpu

ORDER = ("eye", "center", "up", "fov", "near", "far")
WANTED = {"cameras": (), "cameras+vertices": ("vertices",),
          "everything": ("vertices", "normals", "diffuse", "light_positions", "light_intensities")}
NO_BARY = "ShadeFoldLaneNoBaryFn"


class _CountCalls:
    def __init__(self, name):
        self.name, self.calls = name, 0

    def __enter__(self):
        self.real = getattr(_native, self.name)

        def counted(*a, **k):
            self.calls += 1
            return self.real(*a, **k)
        setattr(_native, self.name, counted)
        return self

    def __exit__(self, *exc):
        setattr(_native, self.name, self.real)


def _shininess(scene, kind):
    if kind == "image":
        return torch.tensor([3.0, 5.5])
    V = scene["vertices"].shape[1]
    return 1.2 + 3.0 * torch.rand(2, V, generator=torch.Generator().manual_seed(9))


def _host_inputs(name, lights, specular):
    s = th.camera_scene(name)
    host = {k: s[k] for k in ("vertices", "normals", "diffuse", "ambient")}
    host["light_positions"] = s["light_positions"][:, :lights].contiguous()
    host["light_intensities"] = s["light_intensities"][:, :lights].contiguous()
    if specular:
        host["specular"], host["shininess"] = s["specular"], _shininess(s, specular)
    return s, host


def _leaves(s, host, wanted, device):
    t = {k: v.clone().to(device).requires_grad_(k in wanted) for k, v in host.items()}
    cams = {k: s["cameras"][k].clone().to(device).requires_grad_(k in cr.INPUTS) for k in ORDER}
    return t, cams


def _render(s, t, cams, device):
    return mesh_renderer.render(t["vertices"], s["triangles"].to(device), t["normals"], t["diffuse"], cams["eye"],
                                cams["center"], cams["up"], t["light_positions"], t["light_intensities"], s["W"], s["H"],
                                specular_colors=t.get("specular"), shininess_coefficients=t.get("shininess"),
                                ambient_color=t["ambient"], fov_y=cams["fov"], near_clip=cams["near"], far_clip=cams["far"])


@functools.lru_cache(maxsize=None)
def _truth(name, lights, specular, device):
    """One probe render of the scene -> the G-buffer it wrote, the image, a target with the borderline pixels switched off,
    and the float64 truth of mean|image - target| differentiated to everything.  Shared by every case of the scene."""
    s, host = _host_inputs(name, lights, specular)
    W, H = s["W"], s["H"]
    t, cams = _leaves(s, host, ("vertices",), device)
    probe = _render(s, t, cams, device)
    saved = probe.grad_fn.saved_tensors                       # clip, ids, bary, ... of either fused renderer
    clip = saved[0]
    ids, bary, _ = _native.rasterize_forward(clip, s["triangles"].to(device), W, H)
    assert torch.equal(saved[1], ids) and torch.equal(saved[2].view(torch.int32), bary.view(torch.int32))
    image = probe.detach().as_subclass(torch.Tensor).clone()
    xf = camera_utils.clip_space_transforms(*[cams[k].detach() for k in ORDER], W / H, device)
    del probe
    ids_h, bary_h, clip_h = ids.cpu().numpy(), bary.cpu().numpy(), clip.cpu().numpy()
    share = th.coverage(ids_h, bary_h)
    assert th.COVERAGE[0] <= share.min() and share.max() <= th.COVERAGE[1], share
    n = lambda k: host[k].numpy()
    spec = dict(specular=n("specular"), shininess=n("shininess"), camera_position=s["cameras"]["eye"].numpy()) if specular else {}
    shade_args = (s["triangles"].numpy(), n("normals"), n("vertices"), n("diffuse"), n("light_positions"),
                  n("light_intensities"), n("ambient"))
    off = torch.from_numpy(truth64.borderline_pixels(ids_h, bary_h, *shade_args, **spec).copy()).to(device)
    target = torch.rand(image.shape, generator=torch.Generator().manual_seed(3)).to(device)
    target[off] = image[off]
    upstream = torch.sign(image - target).cpu().numpy().astype(np.float64) / image.numel()
    T = th.scene_truth(ids_h, bary_h, clip_h, xf.cpu().numpy(), shade_args[0], *shade_args[1:], upstream, **spec)
    chain = th.camera_chain_truth(s["cameras"], W / H, n("vertices"), T["d_clip"], T["noise_clip"],
                                  T["d_camera"] if specular else None, T.get("noise_camera"))
    for k in cr.INPUTS:
        assert float(np.abs(chain[k][0]).max()) > 0, k
    return {"image": image, "target": target, "truth": T, "chain": chain, "off": int(off.sum())}


def _check(label, got, want, noise, worst):
    """worst[label] = (excess over the rounding bound, reach): reach is the excess a gradient of all zeros would have --
    how many times its bound the largest element of the truth is, i.e. what a lost term costs."""
    got = got.detach().cpu().numpy()
    worst[label] = (truth64.excess(got, want, noise), truth64.excess(np.zeros_like(want), want, noise))
    assert worst[label][1] > 1.0, "%s: the bound is wider than the gradient itself" % label
    truth64.assert_within_rounding(got, want, noise, label)


def _figures(worst):
    return "  ".join("%s %.2g (of %.2g)" % ((k.rsplit(": d ", 1)[1],) + v) for k, v in worst.items())


def _loss(route, img, target):
    if route == "generic_op":
        losses.USE_FUSED_RENDER_LOSS = False
        try:
            return losses.l1_loss(img, target)
        finally:
            losses.USE_FUSED_RENDER_LOSS = True
    if route == "mean_abs":
        return torch.mean(torch.abs(img - target))
    return losses.l1_loss(img, target)


def _case(device, name, wanted, route, lights=2, specular=None):
    """One differentiated render of the scene -> (camera leaves, other leaves, the accumulate kernel that ran)."""
    ref = _truth(name, lights, specular, device)
    s, host = _host_inputs(name, lights, specular)
    t, cams = _leaves(s, host, WANTED[wanted], device)
    if route == "remembered":
        losses.remember_target(ref["target"])
    try:
        with _CountCalls("l1_loss_forward") as counter:
            img = _render(s, t, cams, device)
            assert torch.equal(img.detach().as_subclass(torch.Tensor), ref["image"])
            loss = _loss(route, img, ref["target"])
        if route == "remembered" and not specular:
            assert counter.calls == 0      # the loss came out of the forward pass
        loss.backward()
        torch.cuda.synchronize()
    finally:
        if route == "remembered":
            losses.forget_target(ref["target"])
    kernel = _native.debug_last_accumulate_kernel()
    label = "%s %s %s L=%d%s" % (name, wanted, route, lights, " specular/" + specular if specular else "")
    worst = {}
    T, chain = ref["truth"], ref["chain"]
    for k in cr.INPUTS:
        assert cams[k].grad is not None and cams[k].grad.shape == (2, 3), k
        _check("%s: d %s" % (label, k), cams[k].grad, chain[k][0], chain[k][1], worst)
    for k in ("vertices", "normals", "diffuse"):
        if k in WANTED[wanted]:
            _check("%s: d %s" % (label, k), t[k].grad, T["d_" + k], T["noise_" + k], worst)
    print("%-60s %-28s excess %s" % (label, kernel.split("(")[0][:28], _figures(worst)))
    return cams, t, kernel


@pytest.mark.parametrize("route", ["l1_loss", "generic_op", "remembered", "mean_abs"])
@pytest.mark.parametrize("wanted", list(WANTED))
@pytest.mark.parametrize("name", th.CAMERA_SCENES)
def test_diffuse_render_camera_gradients(device, name, wanted, route):
    _, _, kernel = _case(device, name, wanted, route)
    assert NO_BARY not in kernel     # a camera gradient needs d clip: never the private G-buffer's kernel


@pytest.mark.parametrize("name", th.CAMERA_SCENES)
def test_deterministic_mode_camera_gradients_are_within_the_same_bound_and_bit_equal(device, name):
    before = _native.set_deterministic(True)
    try:
        runs = [_case(device, name, "cameras+vertices", "l1_loss") for _ in range(2)]
    finally:
        _native.set_deterministic(before)
    (cams_a, t_a, _), (cams_b, t_b, _) = runs
    for k in cr.INPUTS:
        assert torch.equal(cams_a[k].grad, cams_b[k].grad), k
    assert torch.equal(t_a["vertices"].grad, t_b["vertices"].grad)


@pytest.mark.parametrize("wanted", list(WANTED))
@pytest.mark.parametrize("shininess", ["image", "vertex"])
@pytest.mark.parametrize("lights", [1, 2, 3])
def test_specular_render_camera_gradients(device, lights, shininess, wanted):
    """The eye feeds both the transform and the view vector; FusedSpecularPhongRenderer gets transforms=None and must run
    an unfolded pixel pass (d clip on its own) whenever a camera requires grad."""
    name = ("cube", "sphere", "soup")[lights - 1]
    for route in ("l1_loss", "generic_op"):
        _, _, kernel = _case(device, name, wanted, route, lights=lights, specular=shininess)
        assert kernel.startswith("Spec"), kernel
        folded = kernel.startswith("SpecCoupledLaneFn") or (kernel.startswith("SpecFoldLaneFn") and kernel.endswith("true>"))
        assert not folded, kernel


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("name", th.CAMERA_SCENES)
def test_rasterize_with_device_cameras_and_six_attributes(device, name, shared):
    """rasterize() on transforms from clip_space_transforms: truth64.interpolate -> raster_pullback -> the same chain.
    shared: camera_up as [3] and camera_lookat as [1,3], expanded inside _device_cameras -- their gradients arrive summed
    over the batch, in the shape they were passed in."""
    s = th.camera_scene(name)
    W, H = s["W"], s["H"]
    cam_h = {k: v.clone() for k, v in s["cameras"].items()}
    if shared:   # image 0's centre and up for both images (still 5 to 95 % covered: asserted below)
        cam_h["center"], cam_h["up"] = cam_h["center"][:1].expand(2, 3).contiguous(), cam_h["up"][:1].expand(2, 3).contiguous()
    g = torch.Generator().manual_seed(21)
    V = s["vertices"].shape[1]
    attrs_h = torch.randn(2, V, 6, generator=g)
    dout_h = torch.randn(2, H, W, 6, generator=g) / (H * W)
    cams = {k: cam_h[k].clone().to(device).requires_grad_(k in cr.INPUTS) for k in ORDER}
    if shared:
        cams["center"] = cam_h["center"][:1].clone().to(device).requires_grad_(True)     # [1,3]
        cams["up"] = cam_h["up"][0].clone().to(device).requires_grad_(True)              # [3]
    vertices = s["vertices"].clone().to(device).requires_grad_(True)
    attrs = attrs_h.to(device).requires_grad_(True)
    tris = s["triangles"].to(device)
    with _CountCalls("camera_transforms") as counter:
        xf = camera_utils.clip_space_transforms(*[cams[k] for k in ORDER], W / H, device)
    assert counter.calls == 1 and xf.shape == (2, 4, 4)
    out = mesh_renderer.rasterize(vertices, attrs, tris, xf, W, H, torch.zeros(6, device=device))
    clip, ids, bary = out.grad_fn.saved_tensors[:3]
    (out * dout_h.to(device)).sum().backward()
    ids_h, bary_h = ids.cpu().numpy(), bary.cpu().numpy()
    share = th.coverage(ids_h, bary_h)
    assert th.COVERAGE[0] <= share.min() and share.max() <= th.COVERAGE[1], share
    T = truth64.interpolate(ids_h, bary_h, s["triangles"].numpy(), attrs_h.numpy(), dout_h.numpy())
    d_clip, noise_clip = truth64.raster_pullback(clip.cpu().numpy(), s["triangles"].numpy(), ids_h, bary_h, T["dbary"], T["gabs"])
    chain = th.camera_chain_truth(cam_h, W / H, s["vertices"].numpy(), d_clip, noise_clip)
    zero = np.zeros(s["vertices"].shape)
    d_vertices, noise_vertices = truth64.whole_vertex_gradient(xf.detach().cpu().numpy(), zero, d_clip, zero, noise_clip)
    label, worst = "%s rasterize()%s" % (name, " shared" if shared else ""), {}
    for k in cr.INPUTS:
        want, noise = chain[k]
        if shared and k != "eye":
            want, noise = want.sum(0, keepdims=True), noise.sum(0, keepdims=True)
            want, noise = (want[0], noise[0]) if k == "up" else (want, noise)
        assert cams[k].grad is not None and tuple(cams[k].grad.shape) == want.shape, (k, cams[k].grad.shape)
        assert float(np.abs(want).max()) > 0
        _check("%s: d %s" % (label, k), cams[k].grad, want, noise, worst)
    _check("%s: d vertices" % label, vertices.grad, d_vertices, noise_vertices, worst)
    _check("%s: d attributes" % label, attrs.grad, T["d_attributes"], T["noise_attributes"], worst)
    print("%-60s excess %s" % (label, _figures(worst)))
