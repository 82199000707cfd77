"""Bilinear texture mapping on the MI355X: the HIP sampler against the float64 restatement (values, both gradients,
every footprint regime of the texture scatter, full size, determinism), render_textured against the same
composition built here from the package's rasterizer and interpolator, graph capture and the example."""
import importlib
import importlib.util
import itertools
import math
import os

import pytest
import torch

import sh_reference
import texture_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import camera_utils, shapes
from pytorch_mesh_renderer_amd.mesh_renderer.rasterize_triangles_ext import AttributeInterpolator, BarycentricRasterizer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# the blend is four binary32 products and three sums of weights <= 1: within 8 ulp of max|tex| of the float64 value
BLEND_ROUNDING = 8 * 2.0 ** -24


def _uv(B, H, W, Ht, Wt, seed, lo=-1.5, hi=2.5):
    """Random UVs in [lo, hi) plus exact texel centres and edges, negative and > 1 coordinates, non-finite ones
    and ones beyond 2^24 texels."""
    g = torch.Generator().manual_seed(seed)
    uv = lo + (hi - lo) * torch.rand(B, H, W, 2, generator=g)
    n = H * W
    flat = uv.view(B, n, 2)
    k = torch.randint(-2 * max(Ht, Wt), 2 * max(Ht, Wt), (B, n, 2), generator=g).float()
    centre = torch.stack([(k[..., 0] + 0.5) / Wt, (k[..., 1] + 0.5) / Ht], -1)
    edge = torch.stack([k[..., 0] / Wt, k[..., 1] / Ht], -1)
    pick = torch.randint(0, 8, (B, n), generator=g)
    flat[pick == 1] = centre[pick == 1]
    flat[pick == 2] = edge[pick == 2]
    flat[:, 0, 0] = float("nan")
    flat[:, 1, 1] = float("inf")
    flat[:, 2, 0] = -float("inf")
    flat[:, 3, 0] = 2.0 ** 25 / Wt
    flat[:, 4, 1] = -(2.0 ** 25) / Ht
    flat[:, 5, 0] = (2.0 ** 24 - 1.0) / Wt       # just inside: x = 2^24 - 1.5 rounds to a valid coordinate
    return uv.to(DEV)


def _tex(batched, B, Ht, Wt, C, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (B, Ht, Wt, C) if batched else (Ht, Wt, C)
    return (torch.rand(shape, generator=g) * 4.0 - 2.0).to(DEV)


def _mask(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor([0.0, 0.5, 0.51, 1.0])[torch.randint(0, 4, (B, H, W), generator=g)].to(DEV)


SIZES = [(5, 7), (1, 1), (3, 1), (13, 6), (1, 9)]          # (Ht, Wt): odd, Ht != Wt, one texel wide or tall
CASES = list(itertools.product([1, 2, 3, 4], [False, True], ["wrap", "clamp"], [False, True]))


@pytest.mark.parametrize("C, batched, boundary, masked", CASES)
def test_values_match_the_restatement(C, batched, boundary, masked):
    Ht, Wt = SIZES[(C + 2 * batched + 3 * masked) % len(SIZES)]
    B, H, W = 2, 37, 70
    tex = _tex(batched, B, Ht, Wt, C, C)
    uv = _uv(B, H, W, Ht, Wt, 10 + C)
    mask = _mask(B, H, W, 20 + C) if masked else None
    out = mesh_renderer.texture(tex, uv, mask, boundary)
    want = ref.sample(tex, uv, mask, boundary)
    assert out.shape == (B, H, W, C) and out.dtype == torch.float32
    tol = (1e-6 + BLEND_ROUNDING) * float(tex.abs().max())
    assert float((out.double() - want).abs().max()) <= tol
    valid = ref.taps(uv, Ht, Wt, mask, boundary)[0]
    assert bool((out[~valid] == 0).all())


def _check_gradients(tex, uv, mask, boundary, dout, want_tex=True, want_uv=True):
    Ht, Wt = tex.shape[-3], tex.shape[-2]
    t = tex.clone().requires_grad_(want_tex)
    q = uv.clone().requires_grad_(want_uv)
    out = mesh_renderer.texture(t, q, mask, boundary)
    out.backward(dout)
    _, dtex, duv, abs_sum = ref.sample(tex, uv, mask, boundary, dout)
    if want_tex:
        err = (t.grad.double() - dtex).abs()
        assert bool((err <= 1e-5 * abs_sum).all()), float((err - 1e-5 * abs_sum).max())
    else:
        assert t.grad is None
    if want_uv:
        tol = 1e-5 * max(Ht, Wt) * float(dout.abs().max()) * float(tex.abs().max())
        assert float((q.grad.double() - duv).abs().max()) <= tol
    else:
        assert q.grad is None


@pytest.mark.parametrize("C, batched, boundary, masked", CASES)
def test_gradients_match_the_restatement(C, batched, boundary, masked):
    Ht, Wt = SIZES[(C + batched + masked) % len(SIZES)]
    B, H, W = 2, 41, 67
    tex = _tex(batched, B, Ht, Wt, C, 30 + C)
    uv = _uv(B, H, W, Ht, Wt, 40 + C)
    mask = _mask(B, H, W, 50 + C) if masked else None
    dout = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(60 + C)).to(DEV)
    _check_gradients(tex, uv, mask, boundary, dout)


@pytest.mark.parametrize("want_tex, want_uv", [(True, False), (False, True), (True, True)])
def test_each_gradient_alone_and_both(want_tex, want_uv):
    B, H, W, Ht, Wt, C = 3, 50, 90, 17, 23, 3
    tex = _tex(False, B, Ht, Wt, C, 70)
    uv = _uv(B, H, W, Ht, Wt, 71, 0.0, 1.0)
    dout = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(72)).to(DEV)
    _check_gradients(tex, uv, _mask(B, H, W, 73), "wrap", dout, want_tex, want_uv)


@pytest.mark.parametrize("batched", [False, True])
def test_a_tiny_texture_under_a_large_image(batched):
    # every pixel adds into the same four texels: the LDS window at its most contended
    B, H, W = 8, 256, 256
    tex = _tex(batched, B, 2, 2, 3, 80)
    uv = _uv(B, H, W, 2, 2, 81, -0.5, 1.5)
    dout = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(82)).to(DEV)
    for boundary in ("wrap", "clamp"):
        _check_gradients(tex, uv, None, boundary, dout)


def test_a_huge_texture_under_random_uvs_takes_the_fallback():
    # 4096^2 texels under 128^2 random UVs: a tile's footprint is the whole texture
    B, H, W, S = 2, 128, 128, 4096
    tex = _tex(False, B, S, S, 3, 90)
    uv = torch.rand(B, H, W, 2, generator=torch.Generator().manual_seed(91)).to(DEV)
    dout = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(92)).to(DEV)
    _check_gradients(tex, uv, None, "wrap", dout)
    _check_gradients(tex, uv, _mask(B, H, W, 93), "clamp", dout)


@pytest.mark.parametrize("C, boundary", itertools.product([1, 2, 4], ["wrap", "clamp"]))
def test_the_fallback_at_every_other_channel_count(C, boundary):
    # one 64 x 16 tile of uniform random UVs over 256^2 texels: its tap box x C is above the LDS window in float and
    # in fixed point, so the leader rounds and the per-lane atomics (unrolled per channel) do all of the scatter
    B, H, W, S = 1, 16, 64, 256
    tex = _tex(False, B, S, S, C, 94)
    uv = torch.rand(B, H, W, 2, generator=torch.Generator().manual_seed(95)).to(DEV)
    dout = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(96)).to(DEV)
    used, cells = _tile_cells(uv.cpu(), None, S, S, C, boundary)
    assert used.shape == (1, 1, 1) and bool(used.all()) and int(cells.min()) > 8192
    _check_gradients(tex, uv, None, boundary, dout)
    before = _native.set_deterministic(True)
    try:
        _check_gradients(tex, uv, None, boundary, dout)
    finally:
        _native.set_deterministic(before)


@pytest.mark.parametrize("batched", [False, True])
def test_tiles_straddling_the_wrap_seam(batched):
    B, H, W, Ht, Wt = 8, 96, 200, 48, 64
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32),
                            indexing="ij")
    shift = torch.arange(B, dtype=torch.float32).view(B, 1, 1) * 0.07
    u = 0.8 + 0.4 * xs / W + shift                            # crosses u = 1 (and 2) inside tiles: continuous
    u = torch.where(ys[None] > H / 2, torch.remainder(u, 1.0), u)  # the lower half jumps from ~1 back to 0
    v = (-0.3 + 0.6 * ys / H).expand(B, H, W)                 # crosses v = 0
    uv = torch.stack([u, v], -1).to(DEV)
    tex = _tex(batched, B, Ht, Wt, 3, 100)
    dout = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(101)).to(DEV)
    out = mesh_renderer.texture(tex, uv, None, "wrap")
    assert float((out.double() - ref.sample(tex, uv, None, "wrap")).abs().max()) <= 1e-5
    _check_gradients(tex, uv, None, "wrap", dout)


def test_full_size_texture_gradient():
    # the benchmark's shape: 1024^2 x 32 images, one shared 1024^2 RGB texture
    B, S, St = 32, 1024, 1024
    g = torch.Generator(device=DEV).manual_seed(110)
    ys, xs = torch.meshgrid(torch.arange(S, device=DEV, dtype=torch.float32),
                            torch.arange(S, device=DEV, dtype=torch.float32), indexing="ij")
    r2 = ((xs - S / 2) ** 2 + (ys - S / 2) ** 2) / (0.45 * S) ** 2
    mask = (r2 < 1.0).float().expand(B, S, S).contiguous()
    offset = torch.rand(B, 1, 1, 2, generator=g, device=DEV)
    uv = torch.stack([xs / S, ys / S], -1).unsqueeze(0) * 1.3 + offset
    tex = torch.rand(St, St, 3, generator=g, device=DEV)
    dout = torch.randn(B, S, S, 3, generator=g, device=DEV)
    t = tex.clone().requires_grad_(True)
    mesh_renderer.texture(t, uv, mask, "wrap").backward(dout)
    _, dtex, _, abs_sum = ref.sample(tex, uv, mask, "wrap", dout)
    err = (t.grad.double() - dtex).abs()
    assert bool((err <= 1e-5 * abs_sum).all()), float((err - 1e-5 * abs_sum).max())


def _tile_cells(uv, mask, Ht, Wt, C, boundary):
    """The backward's 64 x 16 pixel tiles (csrc/texture_taps.h: scatter_level) -> (which tiles sample any texel, each
    tile's tap box x C in cells), from the restatement's taps.  The box is in unwrapped texel indices under wrap,
    clamped ones under clamp."""
    valid = ref.taps(uv, Ht, Wt, mask, boundary)[0]
    x, y = ref._coords(uv, Ht, Wt)
    x0 = torch.floor(torch.where(valid, x, torch.zeros_like(x))).long()
    y0 = torch.floor(torch.where(valid, y, torch.zeros_like(y))).long()
    lo_x, hi_x, lo_y, hi_y = x0, x0 + 1, y0, y0 + 1
    if boundary == "clamp":
        lo_x, hi_x = lo_x.clamp(0, Wt - 1), hi_x.clamp(0, Wt - 1)
        lo_y, hi_y = lo_y.clamp(0, Ht - 1), hi_y.clamp(0, Ht - 1)
    B, H, W = valid.shape
    ph, pw = -H % 16, -W % 64
    big = 1 << 40

    def tiles(t, fill):
        t = torch.nn.functional.pad(torch.where(valid, t, torch.full_like(t, fill)), (0, pw, 0, ph), value=fill)
        return t.view(B, (H + ph) // 16, 16, (W + pw) // 64, 64)
    bx0, by0 = tiles(lo_x, big).amin((2, 4)), tiles(lo_y, big).amin((2, 4))
    bx1, by1 = tiles(hi_x, -big).amax((2, 4)), tiles(hi_y, -big).amax((2, 4))
    return bx0 <= bx1, (bx1 - bx0 + 1) * (by1 - by0 + 1) * C


def _tile_paths(uv, mask, Ht, Wt, C, boundary):
    """-> (tiles that sample any texel, those whose tap box x C fits the bilinear backward's float LDS window (32 KiB:
    8192 cells), those whose box fits its fixed-point window (4096 cells)); the rest take the per-lane fallback."""
    used, cells = _tile_cells(uv, mask, Ht, Wt, C, boundary)
    return int(used.sum()), int((used & (cells <= 8192)).sum()), int((used & (cells <= 4096)).sum())


@pytest.mark.parametrize("Ht, Wt, boundary", [(64, 64, "wrap"), (48, 80, "clamp"), (300, 500, "wrap")])
def test_deterministic_texture_gradient_is_bit_identical_and_matches(Ht, Wt, boundary):
    B, H, W = 4, 200, 300
    uv = _uv(B, H, W, Ht, Wt, 120, 0.0, 1.0)
    ys = torch.arange(H, device=DEV, dtype=torch.float32).view(1, H, 1)
    xs = torch.arange(W, device=DEV, dtype=torch.float32).view(1, 1, W)
    # the upper half smooth (u crosses 1: tiles on the wrap seam, or on the clamped edge), the lower half random
    smooth = torch.stack([(0.6 + 0.8 * xs / W).expand(B, H, W), (ys / H).expand(B, H, W)], -1)
    uv = torch.where((ys < H / 2).unsqueeze(-1), smooth, uv)
    used, fit_float, fit_fixed = _tile_paths(uv, None, Ht, Wt, 3, boundary)
    if Ht == 300:
        assert fit_fixed == 0 < fit_float < used      # float mode: windows and fallback; fixed: fallback only
    else:
        assert 0 < fit_fixed < used                   # fixed point: the LDS window and the fallback both run
    tex = _tex(False, B, Ht, Wt, 3, 121)
    dout = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(122)).to(DEV)
    float_dtex, float_duv = _native.texture_backward(dout, tex, uv, None, boundary)
    before = _native.set_deterministic(True)
    try:
        runs = [_native.texture_backward(dout, tex, uv, None, boundary) for _ in range(2)]
        # a contribution outside the fixed-point range (csrc/det_fixed.h) -- an infinite upstream gradient on one
        # pixel of the smooth half, whose UV is valid, and a NaN -- poisons the whole of dtex (d uv is per pixel)
        for poison in (float("inf"), float("nan")):
            bad = dout.clone()
            bad[1, 10, 10, 1] = poison
            assert not bool(torch.isfinite(_native.texture_backward(bad, tex, uv, None, boundary)[0]).any()), poison
    finally:
        _native.set_deterministic(before)
    assert _native.deterministic() == before
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][1], float_duv)                    # d uv is per pixel in either mode
    _, dtex, _, abs_sum = ref.sample(tex, uv, None, boundary, dout)
    err = (float_dtex.double() - dtex).abs()
    assert bool((err <= 1e-5 * abs_sum).all()), float((err - 1e-5 * abs_sum).max())
    # fixed point (csrc/det_fixed.h): each contribution is rounded to the quantum 2^-k, where 2^k maps the largest |dout|
    # (times max(1, pixels per texture / 2^21)) into [2^40, 2^41): half a quantum of absolute error per contribution
    gain = max(1.0, B * H * W / 2.0 ** 21)
    k = min(max(41 - math.frexp(float(dout.abs().max()) * gain)[1], -100), 100)
    err = (runs[0][0].double() - dtex).abs()
    bound = 1e-5 * abs_sum + 0.5 * 2.0 ** -k * _contributions(uv, Ht, Wt, boundary)
    assert bool((err <= bound).all()), float((err - bound).max())


def _contributions(uv, Ht, Wt, boundary):
    """[Ht,Wt,1]: the number of (pixel, tap) contributions each texel of a shared texture receives."""
    valid, _, _, tp = ref.taps(uv, Ht, Wt, None, boundary)
    count = torch.zeros(Ht * Wt, dtype=torch.float64, device=uv.device)
    for r, c in tp:
        idx = (r * Wt + c)[valid]
        count.index_add_(0, idx, torch.ones(idx.shape[0], dtype=torch.float64, device=uv.device))
    return count.view(Ht, Wt, 1)


# ---- render_textured ---------------------------------------------------------------------------------------------
def _scene(B=2, size=(72, 56), per_vertex=False, batched_texture=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    vertices, triangles, normals = shapes.sphere(1.0, 12)
    if per_vertex:
        uvs = torch.rand(vertices.shape[0], 2, generator=g) * 2.0 - 0.5
        uv_triangles = None
    else:
        uvs, uv_triangles = shapes.sphere_uvs(12)
        uv_triangles = uv_triangles.to(DEV)
    tshape = (B, 9, 14, 3) if batched_texture else (9, 14, 3)
    return {"vertices": (vertices.unsqueeze(0).repeat(B, 1, 1) + 0.05 * torch.randn(B, vertices.shape[0], 3,
                                                                                       generator=g)).to(DEV),
            "triangles": triangles.to(DEV), "normals": normals.unsqueeze(0).repeat(B, 1, 1).to(DEV),
            "uvs": uvs.to(DEV), "uv_triangles": uv_triangles, "texture": torch.rand(tshape, generator=g).to(DEV),
            "sh": (torch.randn(9, 3, generator=g) * 0.2 + torch.tensor([[0.9, 0.9, 0.9]] + [[0.0] * 3] * 8)).to(DEV),
            "eye": torch.tensor([[0.3, 0.8, 3.0], [-2.5, 0.4, 1.8]][:B], device=DEV),
            "width": size[0], "height": size[1]}


def _composed(s, vertices, uvs, texture, normals, sh, boundary, antialias):
    """render_textured restated from the package's rasterizer / interpolator, the float64 sampler and the float64
    SH shading."""
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
    albedo = ref.sample(texture, px[..., 0:2], alpha, boundary)
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
            image = mesh_renderer.render_textured(
                leaves["vertices"], s["triangles"], leaves["uvs"], leaves["texture"], s["eye"], torch.zeros(3, device=DEV),
                torch.tensor([0.0, 1.0, 0.0], device=DEV), s["width"], s["height"], uv_triangles=s["uv_triangles"],
                normals=s["normals"], sh_coefficients=sh, boundary_mode=boundary, antialias=antialias)
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


def test_render_textured_with_sh_needs_no_more_than_the_shading():
    # rgb = albedo * SH irradiance, and the unlit colour is the albedo: a constant-irradiance light scales it
    s = _scene(seed=7)
    dc = torch.zeros(9, 3, device=DEV)
    dc[0] = 2.0 / 0.282094791773878
    args = (s["vertices"], s["triangles"], s["uvs"], s["texture"], s["eye"], torch.zeros(3, device=DEV),
            torch.tensor([0.0, 1.0, 0.0], device=DEV), s["width"], s["height"])
    unlit = mesh_renderer.render_textured(*args, uv_triangles=s["uv_triangles"])
    lit = mesh_renderer.render_textured(*args, uv_triangles=s["uv_triangles"], normals=s["normals"],
                                        sh_coefficients=dc)
    torch.testing.assert_close(lit[..., :3], 2.0 * unlit[..., :3], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(lit[..., 3], unlit[..., 3])


def test_captured_step_replays_to_the_eager_result():
    s = _scene(seed=8)
    vertices = s["vertices"].clone().requires_grad_(True)
    texture = s["texture"].clone().requires_grad_(True)
    uvs = s["uvs"].clone().requires_grad_(True)
    target = torch.rand(2, s["height"], s["width"], 4, generator=torch.Generator().manual_seed(9)).to(DEV)
    center, up = torch.zeros(2, 3, device=DEV), torch.tensor([[0.0, 1.0, 0.0]], device=DEV).repeat(2, 1)

    def step():
        image = mesh_renderer.render_textured(vertices, s["triangles"], uvs, texture, s["eye"], center, up,
                                              s["width"], s["height"], uv_triangles=s["uv_triangles"])
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


def test_example_recovers_the_texture():
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fit_texture", os.path.join(root, "examples", "fit_texture.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    start = time.time()
    result = example.fit(steps=200, size=64, device=DEV)
    assert time.time() - start < 60.0, result
    assert result["final_loss"] <= 1e-2 * result["initial_loss"], result
    assert result["final_texel_error"] <= 0.1 * result["initial_texel_error"], result
    assert result["seen_texels"] >= 1000, result
