"""Mipmapped trilinear texture mapping on the MI355X: the HIP pyramid, sampler and screen-space derivatives against
their restatements (tests/texture_mip_reference.py) -- pyramid bits, values, both gradients, every footprint regime
of the per-level texture scatter, determinism -- render_textured_filtered in mipmap mode against the same composition built
here, graph capture and the example."""
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

import sh_reference
import texture_mip_reference as ref
import texture_reference
from conftest import golden_npz
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import camera_utils, shapes
from pytorch_mesh_renderer_amd.mesh_renderer.rasterize_triangles_ext import AttributeInterpolator, BarycentricRasterizer
from test_texture_gpu import _mask, _tex, _tile_cells, _uv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MIP = "linear-mipmap-linear"
# Two bilinear blends of 8 ulp each and the lerp: 20 ulp of max|tex|.  The lod is off by at most ~1.3e-6 (relative
# rounding of rho^2 through log2: <= 3e-7; one ulp of log2f at a magnitude <= 32, halved: <= 1e-6), times
# |c1 - c0| <= 2 max|tex|: <= 2.6e-6 max|tex|.
VALUE_TOL = 4e-6 + 20 * 2.0 ** -24
SIZES = [(16, 32), (12, 20), (8, 8), (5, 7)]               # L = 5, 3, 4, 1
CASES = list(itertools.product([1, 2, 3, 4], [False, True], ["wrap", "clamp"], [False, True]))


def _uv_da(B, H, W, Ht, Wt, seed):
    """Footprints whose lod runs log-uniformly from -3 to L + 2, any orientation and sign, plus exact zeros, exact
    powers of two (an integer lod when the extent is a power of two), NaN and +-inf entries."""
    g = torch.Generator().manual_seed(seed)
    L = ref.levels(Ht, Wt)
    n = H * W
    rho = 2.0 ** (-3.0 + (L + 5.0) * torch.rand(B, n, generator=g))
    theta = 6.2831853 * torch.rand(B, n, generator=g)
    minor = torch.rand(B, n, generator=g) * (torch.randint(0, 2, (B, n), generator=g) * 2.0 - 1.0)
    da = torch.stack([rho * torch.cos(theta) / Wt, -minor * rho * torch.sin(theta) / Wt,
                      rho * torch.sin(theta) / Ht, minor * rho * torch.cos(theta) / Ht], -1)
    swap = torch.randint(0, 2, (B, n), generator=g).bool()
    da = torch.where(swap.unsqueeze(-1), da[..., [1, 0, 3, 2]], da)
    pick = torch.randint(0, 10, (B, n), generator=g)
    da[pick == 1] = 0.0
    k = torch.randint(-2, L + 2, (B, n), generator=g).float()
    power = torch.zeros(B, n, 4)
    power[..., 0] = -(2.0 ** k) / Wt
    da[pick == 2] = power[pick == 2]
    power = torch.zeros(B, n, 4)
    power[..., 3] = 2.0 ** k / Ht
    da[pick == 3] = power[pick == 3]
    da[:, 7, 0] = float("nan")
    da[:, 8, 3] = float("nan")
    da[:, 9, 1] = float("inf")
    da[:, 10, 2] = -float("inf")
    da[:, 11] = torch.tensor([float("inf"), 0.0, float("nan"), 0.0])
    return da.view(B, H, W, 4).to(DEV)


@pytest.mark.parametrize("C, batched", itertools.product([1, 2, 3, 4], [False, True]))
def test_pyramid_is_bit_identical_to_the_float32_restatement(C, batched):
    for Ht, Wt in [(8, 8), (12, 20), (64, 2), (5, 7)]:
        tex = _tex(batched, 3, Ht, Wt, C, 1 + C)
        got = _native.texture_mip_pyramid(tex)
        want = ref.pyramid(tex.cpu())[1:]
        assert len(got) == len(want) == ref.levels(Ht, Wt) - 1 == mesh_renderer.texture_mip_levels(Ht, Wt) - 1
        for lg, lw in zip(got, want):
            lw = lw if batched else lw.unsqueeze(0)
            assert lg.shape == lw.shape
            assert torch.equal(lg.cpu(), lw)
    capped = _native.texture_mip_pyramid(_tex(batched, 3, 8, 8, C, 9), max_mip_level=1)
    assert len(capped) == 1 and capped[0].shape[1:3] == (4, 4)


@pytest.mark.parametrize("C, batched, boundary, masked", CASES)
def test_values_match_the_restatement(C, batched, boundary, masked):
    Ht, Wt = SIZES[(C + 2 * batched + 3 * masked) % len(SIZES)]
    B, H, W = 2, 37, 70
    tex = _tex(batched, B, Ht, Wt, C, C)
    uv = _uv(B, H, W, Ht, Wt, 10 + C)
    uv_da = _uv_da(B, H, W, Ht, Wt, 15 + C)
    mask = _mask(B, H, W, 20 + C) if masked else None
    out = mesh_renderer.texture_filtered(tex, uv, mask, boundary, uv_da, MIP)
    want = ref.sample(tex, uv, uv_da, mask, boundary)
    assert out.shape == (B, H, W, C) and out.dtype == torch.float32
    err = float((out.double() - want).abs().max())
    print("max error %.3g of %.3g" % (err, VALUE_TOL * float(tex.abs().max())))
    assert err <= VALUE_TOL * float(tex.abs().max())
    valid = texture_reference.taps(uv, Ht, Wt, mask, boundary)[0]
    assert bool((out[~valid] == 0).all())


def test_a_capped_pyramid_samples_the_levels_it_has():
    B, H, W, Ht, Wt = 2, 37, 70, 16, 32
    tex, uv, uv_da = _tex(False, B, Ht, Wt, 3, 3), _uv(B, H, W, Ht, Wt, 4), _uv_da(B, H, W, Ht, Wt, 5)
    for cap in (0, 2, 99):
        out = mesh_renderer.texture_filtered(tex, uv, None, "wrap", uv_da, MIP, cap)
        want = ref.sample(tex, uv, uv_da, None, "wrap", cap)
        assert float((out.double() - want).abs().max()) <= VALUE_TOL * float(tex.abs().max())
    assert torch.equal(mesh_renderer.texture_filtered(tex, uv, None, "wrap", uv_da, MIP, 0), mesh_renderer.texture(tex, uv))


@pytest.mark.parametrize("C, boundary", itertools.product([1, 2, 3, 4], ["wrap", "clamp"]))
def test_zero_derivatives_and_one_level_textures_equal_the_bilinear_op(C, boundary):
    B, H, W = 2, 37, 70
    for Ht, Wt in SIZES:
        tex, uv, mask = _tex(C % 2 == 0, B, Ht, Wt, C, 30), _uv(B, H, W, Ht, Wt, 31), _mask(B, H, W, 32)
        bilinear = mesh_renderer.texture(tex, uv, mask, boundary)
        zero = torch.zeros(B, H, W, 4, device=DEV)
        assert torch.equal(mesh_renderer.texture_filtered(tex, uv, mask, boundary, zero, MIP), bilinear)
        if ref.levels(Ht, Wt) == 1:
            assert torch.equal(mesh_renderer.texture_filtered(tex, uv, mask, boundary, _uv_da(B, H, W, Ht, Wt, 33), MIP), bilinear)


def _check_gradients(tex, uv, uv_da, mask, boundary, dout, want_tex=True, want_uv=True, max_mip_level=None, got=None):
    Ht, Wt = tex.shape[-3], tex.shape[-2]
    if got is None:
        t = tex.clone().requires_grad_(want_tex)
        q = uv.clone().requires_grad_(want_uv)
        da = uv_da.clone().requires_grad_(True)
        mesh_renderer.texture_filtered(t, q, mask, boundary, da, MIP, max_mip_level).backward(dout)
        assert da.grad is None
        got = (t.grad, q.grad)
    _, dtex, duv, abs_sum = ref.sample(tex, uv, uv_da, mask, boundary, max_mip_level, dout)
    if want_tex:
        err = (got[0].double() - dtex).abs()
        print("d tex: worst error / (1e-5 abs_sum) = %.3g" % float((err / (1e-5 * abs_sum).clamp_min(1e-300)).max()))
        assert bool((err <= 1e-5 * abs_sum).all()), float((err - 1e-5 * abs_sum).max())
    else:
        assert got[0] is None
    if want_uv:
        tol = 1e-5 * max(Ht, Wt) * float(dout.abs().max()) * float(tex.abs().max())
        assert float((got[1].double() - duv).abs().max()) <= tol
    else:
        assert got[1] is None


@pytest.mark.parametrize("C, batched, boundary, masked", CASES)
def test_gradients_match_the_restatement(C, batched, boundary, masked):
    Ht, Wt = SIZES[(C + batched + masked) % len(SIZES)]
    B, H, W = 2, 41, 67
    tex = _tex(batched, B, Ht, Wt, C, 40 + C)
    uv = _uv(B, H, W, Ht, Wt, 45 + C)
    uv_da = _uv_da(B, H, W, Ht, Wt, 50 + C)
    mask = _mask(B, H, W, 55 + C) if masked else None
    dout = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(60 + C)).to(DEV)
    _check_gradients(tex, uv, uv_da, mask, boundary, dout)


@pytest.mark.parametrize("want_tex, want_uv", [(True, False), (False, True), (True, True)])
def test_each_gradient_alone_and_both(want_tex, want_uv):
    B, H, W, Ht, Wt, C = 2, 41, 67, 16, 32, 3
    tex = _tex(False, B, Ht, Wt, C, 70)
    uv = _uv(B, H, W, Ht, Wt, 71, 0.0, 1.0)
    dout = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(72)).to(DEV)
    _check_gradients(tex, uv, _uv_da(B, H, W, Ht, Wt, 74), _mask(B, H, W, 73), "wrap", dout, want_tex, want_uv)


def _pixel_grid(B, H, W):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return ys.expand(B, H, W), xs.expand(B, H, W)


@pytest.mark.parametrize("batched", [False, True])
def test_a_tiny_texture_under_a_large_image(batched):
    # a 4 x 4 texture (L = 3) with lod >= 2 everywhere: every pixel adds into the one texel of level 2
    B, H, W = 8, 256, 256
    tex = _tex(batched, B, 4, 4, 3, 80)
    uv = _uv(B, H, W, 4, 4, 81, -0.5, 1.5)
    g = torch.Generator().manual_seed(83)
    uv_da = torch.zeros(B, H, W, 4)
    uv_da[..., 0] = 2.0 ** (2.0 + 2.0 * torch.rand(B, H, W, generator=g)) / 4
    uv_da[..., 3] = 2.0 ** (4.0 * torch.rand(B, H, W, generator=g) - 1.0) / 4
    dout = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(82)).to(DEV)
    assert int(ref.lod(uv_da, 4, 4, 3)[0].min()) == 2
    for boundary in ("wrap", "clamp"):
        _check_gradients(tex, uv, uv_da.to(DEV), None, boundary, dout)


def test_a_huge_texture_under_random_uvs_takes_the_fallback():
    # 2048^2 texels under 128^2 random UVs at a 16 x minification: a tile's footprint is the whole of level 4 (128^2)
    B, H, W, S = 2, 128, 128, 2048
    tex = _tex(False, B, S, S, 3, 90)
    uv = torch.rand(B, H, W, 2, generator=torch.Generator().manual_seed(91)).to(DEV)
    uv_da = torch.zeros(B, H, W, 4, device=DEV)
    uv_da[..., 0] = 16.0 / S
    uv_da[..., 3] = 15.0 / S
    dout = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(92)).to(DEV)
    _check_gradients(tex, uv, uv_da, None, "wrap", dout)
    # lod clamped at 0 by a capped pyramid: the scatter goes to level 0 itself, all of it
    _check_gradients(tex, uv, uv_da, _mask(B, H, W, 93), "clamp", dout, max_mip_level=0)


@pytest.mark.parametrize("C, boundary", itertools.product([1, 2, 4], ["wrap", "clamp"]))
def test_the_fallback_at_every_other_channel_count(C, boundary):
    # one 64 x 16 tile of uniform random UVs over 256^2 texels with zero derivatives (lod 0: the scatter lands on
    # level 0): its tap box x C is above the 60 KiB LDS window (15360 float cells) in float and in fixed point, so the
    # leader rounds and the per-lane atomics (unrolled per channel) do all of the scatter
    B, H, W, S = 1, 16, 64, 256
    tex = _tex(False, B, S, S, C, 94)
    uv = torch.rand(B, H, W, 2, generator=torch.Generator().manual_seed(95)).to(DEV)
    uv_da = torch.zeros(B, H, W, 4, device=DEV)
    dout = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(96)).to(DEV)
    used, cells = _tile_cells(uv.cpu(), None, S, S, C, boundary)
    assert used.shape == (1, 1, 1) and bool(used.all()) and int(cells.min()) > 15360
    _check_gradients(tex, uv, uv_da, None, boundary, dout)
    before = _native.set_deterministic(True)
    try:
        _check_gradients(tex, uv, uv_da, None, boundary, dout)
    finally:
        _native.set_deterministic(before)


@pytest.mark.parametrize("batched", [False, True])
def test_tiles_straddling_the_wrap_seam_at_levels_0_and_2(batched):
    B, H, W, Ht, Wt = 4, 96, 200, 48, 64
    ys, xs = _pixel_grid(B, H, W)
    shift = torch.arange(B, dtype=torch.float32).view(B, 1, 1) * 0.07
    u = 0.8 + 0.4 * xs / W + shift                             # crosses u = 1 (and 2) inside tiles: continuous
    u = torch.where(ys > H / 2, torch.remainder(u, 1.0), u)    # the lower half jumps from ~1 back to 0
    v = -0.3 + 0.6 * ys / H                                    # crosses v = 0
    uv = torch.stack([u, v], -1).to(DEV)
    uv_da = torch.zeros(B, H, W, 4)
    uv_da[..., 0] = 0.4 / W                                    # the true step: 0.128 texels, lod 0 ...
    uv_da[..., 3] = 0.6 / H
    right = xs >= 64                                           # ... and from the second tile column on, lod 2 .. 2.5
    uv_da[..., 0] = torch.where(right, (4.0 + 1.6 * ys / H) / Wt, uv_da[..., 0])
    tex = _tex(batched, B, Ht, Wt, 3, 100)
    dout = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(101)).to(DEV)
    l0 = ref.lod(uv_da, Ht, Wt, 5)[0]
    assert int(l0[:, :, :64].max()) == 0 and int(l0[:, :, 64:].min()) == 2
    out = mesh_renderer.texture_filtered(tex, uv, None, "wrap", uv_da.to(DEV), MIP)
    want = ref.sample(tex, uv, uv_da.to(DEV), None, "wrap")
    assert float((out.double() - want).abs().max()) <= VALUE_TOL * float(tex.abs().max())
    _check_gradients(tex, uv, uv_da.to(DEV), None, "wrap", dout)


def test_a_tile_whose_lod_spans_three_levels():
    B, H, W, Ht, Wt = 2, 48, 192, 64, 128
    ys, xs = _pixel_grid(B, H, W)
    lod = 0.25 + 2.5 * (xs % 64) / 64 + 0.2 * (ys % 16) / 16   # 0.25 .. 2.95 within every 64 x 16 tile
    step = 2.0 ** lod
    uv = torch.stack([torch.cumsum(step / Wt, 2), 0.1 + torch.cumsum(step / Ht, 1) * 0.5], -1).to(DEV)
    uv_da = torch.zeros(B, H, W, 4)
    uv_da[..., 0] = step / Wt
    uv_da[..., 3] = 0.5 * step / Ht
    l0 = ref.lod(uv_da, Ht, Wt, ref.levels(Ht, Wt))[0]
    assert sorted(l0[0, :16, :64].unique().tolist()) == [0, 1, 2]
    tex = _tex(False, B, Ht, Wt, 3, 110)
    dout = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(111)).to(DEV)
    for boundary in ("wrap", "clamp"):
        _check_gradients(tex, uv, uv_da.to(DEV), None, boundary, dout)


@pytest.mark.parametrize("Ht, Wt, boundary", [(64, 64, "wrap"), (48, 80, "clamp"), (300, 500, "wrap")])
def test_deterministic_texture_gradient_is_bit_identical_and_matches(Ht, Wt, boundary):
    B, H, W = 4, 200, 300
    uv = _uv(B, H, W, Ht, Wt, 120, 0.0, 1.0)
    ys = torch.arange(H, device=DEV, dtype=torch.float32).view(1, H, 1)
    xs = torch.arange(W, device=DEV, dtype=torch.float32).view(1, 1, W)
    # the upper half smooth (u crosses 1: tiles on the wrap seam, or on the clamped edge), the lower half random
    smooth = torch.stack([(0.6 + 0.8 * xs / W).expand(B, H, W), (ys / H).expand(B, H, W)], -1)
    uv = torch.where((ys < H / 2).unsqueeze(-1), smooth, uv)
    uv_da = _uv_da(B, H, W, Ht, Wt, 123)
    true_step = torch.tensor([0.8 / W, 0.0, 0.0, 1.0 / H], device=DEV).expand(B, H, W, 4)
    uv_da = torch.where((ys < H / 4).unsqueeze(-1), true_step, uv_da)
    tex = _tex(False, B, Ht, Wt, 3, 121)
    dout = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(122)).to(DEV)
    _, pyramid = _native.texture_mip_forward(tex, uv, uv_da, None, boundary)
    float_dtex, float_duv = _native.texture_mip_backward(dout, tex, pyramid, uv, uv_da, None, boundary)
    before = _native.set_deterministic(True)
    try:
        runs = [_native.texture_mip_backward(dout, tex, pyramid, uv, uv_da, None, boundary) for _ in range(2)]
    finally:
        _native.set_deterministic(before)
    assert _native.deterministic() == before
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][1], float_duv)                    # d uv is per pixel in either mode
    _check_gradients(tex, uv, uv_da, None, boundary, dout, got=(float_dtex, float_duv))
    _check_gradients(tex, uv, uv_da, None, boundary, dout, got=runs[0])


# ---- attribute derivatives ---------------------------------------------------------------------------------------
def _check_derivatives(clip, triangles, attributes, attribute_triangles, W, H):
    """-> the all-float32 formula's largest error / scale against the float64 one (the kernel is allowed 4 x that)."""
    ids, bary, _ = _native.rasterize_forward(clip, triangles, W, H)
    got = mesh_renderer.attribute_derivatives(ids, bary, clip, triangles, attributes, attribute_triangles)
    B, A = clip.shape[0], attributes.shape[-1]
    assert got.shape == (B, H, W, A, 2) and got.dtype == torch.float32
    args = [t.cpu().numpy() for t in (ids, bary, clip, triangles, attributes)]
    args.append(attribute_triangles.cpu().numpy() if attribute_triangles is not None else None)
    want, scale, covered = ref.attribute_derivatives(*args)
    single, _, _ = ref.attribute_derivatives(*args, all_float32=True)
    assert covered.any()
    got = got.cpu().numpy()
    assert (got[~covered] == 0).all()
    on = scale > 0
    ratio32 = float((np.abs(single.astype(np.float64) - want)[on] / scale[on]).max())
    ratio = float((np.abs(got.astype(np.float64) - want)[on] / scale[on]).max())
    print("err / scale: float32 numpy %.3g, kernel %.3g" % (ratio32, ratio))
    assert ratio32 > 0
    assert ratio <= 4 * ratio32
    assert (np.abs(got.astype(np.float64) - want)[~on] == 0).all()
    return ratio32, ratio


def _sphere_clip(B, W, H):
    vertices, triangles, _ = shapes.sphere(1.0, 12)
    eye = torch.tensor([[0.3, 0.8, 3.0], [-2.5, 0.4, 1.8]][:B])
    transforms = camera_utils.clip_space_transforms(
        eye, torch.zeros(B, 3), torch.tensor([0.0, 1.0, 0.0]).repeat(B, 1), torch.full((B,), 40.0),
        torch.full((B,), 0.01), torch.full((B,), 10.0), W / H, torch.device("cpu"))
    clip = camera_utils.transform_homogeneous(transforms, vertices.unsqueeze(0).repeat(B, 1, 1))
    return clip.contiguous().to(DEV), triangles.to(DEV)


def test_attribute_derivatives_on_the_uv_sphere():
    W, H, B = 64, 48, 2
    clip, triangles = _sphere_clip(B, W, H)
    uvs, uv_triangles = shapes.sphere_uvs(12)
    ids, bary, _ = _native.rasterize_forward(clip, triangles, W, H)
    assert bool((bary.sum(-1) == 0).any())                     # there is background, and it is exactly 0 (checked below)
    _check_derivatives(clip, triangles, uvs.unsqueeze(0).repeat(B, 1, 1).to(DEV), uv_triangles.to(DEV), W, H)
    g = torch.Generator().manual_seed(130)
    for A in (1, 3, 4):                                        # per vertex, through `triangles`
        _check_derivatives(clip, triangles, torch.randn(B, clip.shape[1], A, generator=g).to(DEV), None, W, H)


def test_attribute_derivatives_with_the_camera_inside_the_cube():
    data = golden_npz("clip_camera_inside_cube.npz")
    clip = torch.from_numpy(data["clip"]).unsqueeze(0).to(DEV)
    triangles = torch.from_numpy(data["triangles"]).to(DEV)
    assert bool((clip[..., 3] < 0).any())                      # (the cube fills the image: no background here)
    g = torch.Generator().manual_seed(131)
    _check_derivatives(clip, triangles, torch.randn(1, 8, 2, generator=g).to(DEV), None, 160, 120)
    corner_triangles = torch.arange(36, dtype=torch.int32).view(12, 3).to(DEV)
    _check_derivatives(clip, triangles, torch.randn(1, 36, 3, generator=g).to(DEV), corner_triangles, 160, 120)


# ---- render_textured ---------------------------------------------------------------------------------------------
def _scene(B=2, size=(64, 48), per_vertex=False, batched_texture=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    vertices, triangles, normals = shapes.sphere(1.0, 12)
    if per_vertex:
        uvs = torch.rand(vertices.shape[0], 2, generator=g) * 2.0 - 0.5
        uv_triangles = None
    else:
        uvs, uv_triangles = shapes.sphere_uvs(12)
        uv_triangles = uv_triangles.to(DEV)
    tshape = (B, 32, 64, 3) if batched_texture else (32, 64, 3)
    return {"vertices": (vertices.unsqueeze(0).repeat(B, 1, 1) + 0.05 * torch.randn(B, vertices.shape[0], 3,
                                                                                       generator=g)).to(DEV),
            "triangles": triangles.to(DEV), "normals": normals.unsqueeze(0).repeat(B, 1, 1).to(DEV),
            "uvs": uvs.to(DEV), "uv_triangles": uv_triangles, "texture": torch.rand(tshape, generator=g).to(DEV),
            "sh": (torch.randn(9, 3, generator=g) * 0.2 + torch.tensor([[0.9, 0.9, 0.9]] + [[0.0] * 3] * 8)).to(DEV),
            "eye": torch.tensor([[0.3, 0.8, 3.0], [-2.5, 0.4, 1.8]][:B], device=DEV),
            "width": size[0], "height": size[1]}


def _composed(s, vertices, uvs, texture, normals, sh, boundary, antialias):
    """render_textured_filtered in mipmap mode restated from the package's rasterizer, interpolator, attribute_derivatives and
    texture(), and the float64 SH shading."""
    B = vertices.shape[0]
    center, up = torch.zeros(B, 3, device=DEV), torch.tensor([0.0, 1.0, 0.0], device=DEV).repeat(B, 1)
    transforms = camera_utils.clip_space_transforms(
        s["eye"], center, up, torch.full((B,), 40.0, device=DEV), torch.full((B,), 0.01, device=DEV),
        torch.full((B,), 10.0, device=DEV), s["width"] / s["height"], DEV)
    clip = camera_utils.transform_homogeneous(transforms, vertices)
    ids, bary, z = BarycentricRasterizer.apply(clip, s["triangles"], s["width"], s["height"])
    u = uvs if uvs.dim() == 3 else uvs.unsqueeze(0).expand(B, *uvs.shape)
    attrs = torch.cat([u, torch.ones(B, u.shape[1], 1, device=DEV)], 2)
    corners = s["uv_triangles"] if s["uv_triangles"] is not None else s["triangles"]
    px = AttributeInterpolator.apply(ids, bary, attrs, corners, torch.zeros(3, device=DEV))
    alpha = (px[..., 2].detach() > 0.5).float()
    uv_da = mesh_renderer.attribute_derivatives(ids, bary, clip, s["triangles"], uvs, s["uv_triangles"])
    assert not uv_da.requires_grad
    uv_da = uv_da.view(B, s["height"], s["width"], 4)
    assert int(ref.lod(uv_da, 32, 64, 6)[0].max()) >= 1       # the scene does minify
    albedo = mesh_renderer.texture_filtered(texture, px[..., 0:2].contiguous(), alpha, boundary, uv_da, MIP).double()
    if sh is None:
        rgba = torch.cat([albedo, alpha.unsqueeze(3).double()], 3)
    else:
        pn = AttributeInterpolator.apply(ids, bary, normals, s["triangles"], torch.zeros(3, device=DEV))
        rgba = sh_reference.shade(pn, albedo, alpha, sh.expand(B, 9, 3), flip=False)
    if antialias:
        rgba = mesh_renderer.antialias(rgba.float(), clip, s["triangles"], ids, bary, z)
    return torch.flip(rgba, dims=[1])


@pytest.mark.parametrize("lit, per_vertex, batched_texture, antialias", [
    (False, False, False, False), (False, True, True, False), (True, False, True, False), (True, True, False, False),
    (False, False, False, True), (True, False, False, True)])
def test_render_textured_matches_the_composition(lit, per_vertex, batched_texture, antialias):
    s = _scene(per_vertex=per_vertex, batched_texture=batched_texture, seed=5)
    boundary = "clamp" if per_vertex else "wrap"
    R = torch.randn(2, s["height"], s["width"], 4, generator=torch.Generator().manual_seed(6)).to(DEV)
    results = []
    for fn in ("kernel", "composed"):
        leaves = {k: s[k].clone().requires_grad_(True) for k in ("vertices", "uvs", "texture", "sh")}
        sh = leaves["sh"] if lit else None
        if fn == "kernel":
            image = mesh_renderer.render_textured_filtered(
                leaves["vertices"], s["triangles"], leaves["uvs"], leaves["texture"], s["eye"], torch.zeros(3, device=DEV),
                torch.tensor([0.0, 1.0, 0.0], device=DEV), s["width"], s["height"], uv_triangles=s["uv_triangles"],
                normals=s["normals"], sh_coefficients=sh, boundary_mode=boundary, antialias=antialias, filter_mode=MIP)
        else:
            image = _composed(s, leaves["vertices"], leaves["uvs"], leaves["texture"], s["normals"], sh, boundary,
                              antialias)
        (image * R).sum().backward()
        results.append((image.detach().double(), {k: v.grad for k, v in leaves.items()}))
    (got, ggrad), (want, wgrad) = results
    assert got.shape == (2, s["height"], s["width"], 4)
    assert float(got[..., 3].max()) == 1.0 and float(got[..., 3].min()) == 0.0
    assert float((got - want).abs().max()) <= 1e-5
    names = ["vertices", "uvs", "texture"] + (["sh"] if lit else [])
    for k in names:
        scale = float(wgrad[k].abs().max())
        assert scale > 0, k
        assert float((ggrad[k].double() - wgrad[k].double()).abs().max()) <= 2e-4 * scale, k
    if not lit:
        assert ggrad["sh"] is None


def test_render_textured_filtered_without_the_new_keywords_is_render_textured():
    s = _scene(seed=7)
    args = (s["vertices"], s["triangles"], s["uvs"], s["texture"], s["eye"], torch.zeros(3, device=DEV),
            torch.tensor([0.0, 1.0, 0.0], device=DEV), s["width"], s["height"])
    plain = mesh_renderer.render_textured(*args, uv_triangles=s["uv_triangles"])
    filtered = mesh_renderer.render_textured_filtered
    assert torch.equal(plain, filtered(*args, uv_triangles=s["uv_triangles"]))
    assert torch.equal(plain, filtered(*args, uv_triangles=s["uv_triangles"], filter_mode="linear"))
    mip = filtered(*args, uv_triangles=s["uv_triangles"], filter_mode=MIP)
    assert not torch.equal(plain, mip)
    assert torch.equal(plain, filtered(*args, uv_triangles=s["uv_triangles"], filter_mode=MIP, max_mip_level=0))


def test_captured_step_replays_to_the_eager_result():
    s = _scene(seed=8)
    vertices = s["vertices"].clone().requires_grad_(True)
    texture = s["texture"].clone().requires_grad_(True)
    uvs = s["uvs"].clone().requires_grad_(True)
    target = torch.rand(2, s["height"], s["width"], 4, generator=torch.Generator().manual_seed(9)).to(DEV)
    center, up = torch.zeros(2, 3, device=DEV), torch.tensor([[0.0, 1.0, 0.0]], device=DEV).repeat(2, 1)

    def step():
        image = mesh_renderer.render_textured_filtered(vertices, s["triangles"], uvs, texture, s["eye"], center, up,
                                                       s["width"], s["height"], uv_triangles=s["uv_triangles"],
                                                       filter_mode=MIP)
        loss = torch.mean(torch.abs(image - target))
        loss.backward()
        return loss

    before = _native.set_deterministic(True)
    try:
        vertices.grad = texture.grad = uvs.grad = None
        eager_loss = step().detach().clone()
        eager = (vertices.grad.clone(), texture.grad.clone(), uvs.grad.clone())
        assert all(float(e.abs().max()) > 0 for e in eager)
        captured = mesh_renderer.capture_step(step, [vertices, texture, uvs])
        for _ in range(2):
            loss = captured.replay()
            torch.cuda.synchronize()
            assert torch.equal(loss, eager_loss)
            assert torch.equal(texture.grad, eager[1])                 # fixed point: bit-reproducible
            # the vertex and uv gradients pass through mr_interpolate_backward's float atomics
            torch.testing.assert_close(vertices.grad, eager[0], rtol=1e-4, atol=1e-6)
            torch.testing.assert_close(uvs.grad, eager[2], rtol=1e-4, atol=1e-6)
    finally:
        _native.set_deterministic(before)


def test_example_mipmapped_fit_recovers_the_minified_texture_better():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fit_texture_minified",
                                                  os.path.join(root, "examples", "fit_texture_minified.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    bilinear = example.fit("linear", device=DEV)
    mipmapped = example.fit(MIP, device=DEV)
    print("level-2 error: bilinear %.4f, mipmapped %.4f (from %.4f)" % (
        bilinear["final_level2_error"], mipmapped["final_level2_error"], mipmapped["initial_level2_error"]))
    assert mipmapped["final_level2_error"] < bilinear["final_level2_error"], (bilinear, mipmapped)
