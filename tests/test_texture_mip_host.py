"""Mipmapped texture mapping on the host: the restatements of tests/texture_mip_reference.py against independent
statements (avg_pool2d, the bilinear restatement, central differences), and the argument checks of texture_filtered /
render_textured_filtered / attribute_derivatives / the _native wrappers and the C ABI (no GPU needed)."""
import ctypes
import importlib
import inspect

import numpy as np
import pytest
import torch

import oracle
import texture_mip_reference as ref
import texture_reference
from conftest import golden_npz
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from test_texture_host import _off_centre_uv, _render_args, _tex_args

texturing = importlib.import_module("pytorch_mesh_renderer_amd.mesh_renderer.texturing")
MIP = "linear-mipmap-linear"


# ---- pyramid -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size, want", [((8, 8), 4), ((12, 20), 3), ((300, 500), 3), ((5, 7), 1), ((64, 1), 1)])
def test_level_counts(size, want):
    assert ref.levels(*size) == want
    assert mesh_renderer.texture_mip_levels(*size) == want            # the library's count, no GPU needed
    for cap in (0, 1, 99):
        assert ref.levels(*size, cap) == min(want, cap + 1) == mesh_renderer.texture_mip_levels(*size, cap)
    assert len(ref.pyramid(torch.zeros(*size, 2))) == want


def test_pyramid_levels_are_the_box_filter_of_the_level_below():
    g = torch.Generator().manual_seed(1)
    for shape in ((8, 8, 3), (2, 12, 20, 1), (300, 500, 2), (5, 7, 4)):
        tex = torch.randn(*shape, generator=g) * 3.0
        pyr = ref.pyramid(tex)
        assert all(p.dtype == torch.float32 for p in pyr)
        for below, level in zip(pyr[:-1], pyr[1:]):
            b = below.double().reshape(-1, *below.shape[-3:]).permute(0, 3, 1, 2)
            want = torch.nn.functional.avg_pool2d(b, 2).permute(0, 2, 3, 1).reshape(level.shape)
            assert float((level.double() - want).abs().max()) <= 3 * 2.0 ** -24 * float(tex.abs().max())


# ---- sampling ----------------------------------------------------------------------------------------------------
def _random_da(B, H, W, Ht, Wt, seed, lo=-2.0, hi=None):
    g = torch.Generator().manual_seed(seed)
    hi = ref.levels(Ht, Wt) + 1.0 if hi is None else hi
    rho = 2.0 ** (lo + (hi - lo) * torch.rand(B, H, W, generator=g))
    theta = 6.2831853 * torch.rand(B, H, W, generator=g)
    return torch.stack([rho * torch.cos(theta) / Wt, 0.3 * rho * torch.sin(theta) / Wt,
                        rho * torch.sin(theta) / Ht, -0.3 * rho * torch.cos(theta) / Ht], -1)


@pytest.mark.parametrize("boundary", ["wrap", "clamp"])
def test_zero_derivatives_give_the_bilinear_restatement_exactly(boundary):
    B, H, W, Ht, Wt, C = 2, 5, 6, 8, 12, 3
    g = torch.Generator().manual_seed(2)
    tex = torch.randn(B, Ht, Wt, C, generator=g)
    uv = torch.rand(B, H, W, 2, generator=g) * 3.0 - 1.0
    uv[0, 0, 0, 0] = float("nan")
    mask = (torch.rand(B, H, W, generator=g) > 0.2).float()
    dout = torch.randn(B, H, W, C, generator=g)
    got = ref.sample(tex, uv, torch.zeros(B, H, W, 4), mask, boundary, None, dout)
    want = texture_reference.sample(tex, uv, mask, boundary, dout)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # and so does a texture with one level, whatever the derivatives
    odd = torch.randn(5, 7, C, generator=g)
    assert torch.equal(ref.sample(odd, uv, _random_da(B, H, W, 5, 7, 3), mask, boundary),
                       texture_reference.sample(odd, uv, mask, boundary))


def test_a_constant_texture_gives_the_constant_at_any_lod():
    B, H, W, Ht, Wt = 2, 6, 7, 16, 8
    tex = torch.full((Ht, Wt, 2), 0.375)
    uv = torch.rand(B, H, W, 2, generator=torch.Generator().manual_seed(4)) * 4.0 - 2.0
    for boundary in ("wrap", "clamp"):
        value = ref.sample(tex, uv, _random_da(B, H, W, Ht, Wt, 5), None, boundary)
        assert float((value - 0.375).abs().max()) <= 1e-15


def test_a_ramp_in_u_is_reproduced_at_every_lod():
    # tex[i, j] = j is Wt u - 0.5 at the texel centres of every level, and bilinear filtering reproduces a linear
    # function between centres: in the interior of the coarsest level the value is Wt u - 0.5 at any lod.  u = k / 1024
    # keeps the binary32 tap decision exact.
    B, H, W, Ht, Wt = 1, 8, 9, 16, 32
    tex = torch.arange(Wt, dtype=torch.float32).view(1, Wt, 1).expand(Ht, Wt, 1).contiguous()
    L = ref.levels(Ht, Wt)
    g = torch.Generator().manual_seed(6)
    lo, hi = 0.5 / (Wt >> (L - 1)), 1.0 - 0.5 / (Wt >> (L - 1))
    u = torch.randint(int(lo * 1024), int(hi * 1024) + 1, (B, H, W), generator=g).float() / 1024
    uv = torch.stack([u, torch.rand(B, H, W, generator=g)], -1)
    bilinear = texture_reference.sample(tex, uv, None, "clamp")
    torch.testing.assert_close(bilinear[..., 0], (u * Wt - 0.5).double(), rtol=0, atol=1e-12)
    for seed in (7, 8):
        value = ref.sample(tex, uv, _random_da(B, H, W, Ht, Wt, seed, -1.0, L + 1.0), None, "clamp")
        torch.testing.assert_close(value, bilinear, rtol=0, atol=1e-12)


def test_reference_gradients_match_central_differences():
    B, H, W, Ht, Wt, C = 2, 3, 4, 8, 16, 2
    g = torch.Generator().manual_seed(9)
    tex = torch.randn(Ht, Wt, C, generator=g, dtype=torch.float64)
    L = ref.levels(Ht, Wt)
    # at least 0.05 texel from a tap boundary at EVERY level.  x_l + 0.5 = (x_0 + 0.5) / 2^l: with x_0 + 0.5 =
    # 2^(L-1) (cell + 0.5 + d), d in [0.075, 0.095], the fractions of x_l are d, 0.5 + 2 d, 0.5 + 4 d and 8 d - 0.5 from
    # the coarsest level (L = 4) down: 0.075 .. 0.095, 0.65 .. 0.69, 0.8 .. 0.88 and 0.1 .. 0.26
    assert L == 4
    cell = torch.randint(-2, 4, (B, H, W, 2), generator=g).double()
    xy = 2 ** (L - 1) * (cell + 0.575 + 0.02 * torch.rand(B, H, W, 2, generator=g, dtype=torch.float64))
    for l in range(L):
        frac = (xy / 2 ** l - 0.5) % 1.0
        assert bool(((frac > 0.05) & (frac < 0.95)).all())
    uv = torch.stack([xy[..., 0] / Wt, xy[..., 1] / Ht], 3)
    # lods away from the integers, from inside level 0 to beyond the top
    lod = torch.tensor([-0.5, 0.3, 0.6, 1.4, 1.7, 2.35, 2.6, 3.5]).repeat(3).view(B, H, W)
    uv_da = torch.zeros(B, H, W, 4)
    uv_da[..., 0] = 2.0 ** lod / Wt
    uv_da[..., 3] = 0.5 * 2.0 ** lod / Ht
    dout = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    for boundary in ("wrap", "clamp"):
        _, dtex, duv, _ = ref.sample(tex, uv, uv_da, None, boundary, None, dout)

        def loss(t, q):
            return float((ref.sample(t, q, uv_da, None, boundary) * dout).sum())
        # the value is linear in the texture (a float64 texture's pyramid is not rounded to binary32)
        for (i, j, c) in ((0, 0, 0), (2, 5, 1), (7, 15, 0), (4, 9, 1)):
            e = torch.zeros_like(tex)
            e[i, j, c] = 1.0
            fd = (loss(tex + e, uv) - loss(tex - e, uv)) / 2.0
            assert abs(fd - float(dtex[i, j, c])) < 1e-9
        # in u (or v) alone it is linear inside a cell of both levels, so a step of 0.04 level-0 texel is exact but
        # for the binary32 rounding of x
        h = 0.04 / max(Ht, Wt)
        for k in range(2):
            for idx in ((0, 0, 0), (1, 2, 3), (0, 1, 2), (1, 0, 1)):
                d = torch.zeros_like(uv)
                d[idx + (k,)] = h
                fd = (float((ref.sample(tex, uv + d, uv_da, None, boundary) * dout)[idx].sum())
                      - float((ref.sample(tex, uv - d, uv_da, None, boundary) * dout)[idx].sum())) / (2 * h)
                assert abs(fd - float(duv[idx + (k,)])) < 1e-4 * max(1.0, abs(fd)), (boundary, k, idx)


# ---- screen-space derivatives ------------------------------------------------------------------------------------
def _check_against_central_differences(clip, triangles, attributes, W, H, want_constant=False):
    """The restatement (float32 U, e, s and stored barycentrics) against central differences of the float64
    perspective-correct interpolation at px +- h, py +- h; -> the number of pixels compared."""
    ids, bary, _ = oracle.forward(clip[None], triangles, W, H)
    deriv, scale, covered = ref.attribute_derivatives(ids, bary, clip[None], triangles, attributes[None])
    assert covered.any() and (deriv[~covered] == 0).all()
    px, py = ref.pixel_centres(W, H)
    h = 1e-4
    ys, xs = np.nonzero(covered[0])
    pick = np.linspace(0, len(ys) - 1, min(len(ys), 200)).astype(int)
    for iy, ix in zip(ys[pick], xs[pick]):
        c = clip[triangles[ids[0, iy, ix]]].astype(np.float64)
        x, y, w = c[:, 0], c[:, 1], c[:, 3]
        for a in range(attributes.shape[1]):
            v = attributes[triangles[ids[0, iy, ix]], a].astype(np.float64)
            cx, cy = float(px[ix]), float(py[iy])
            dx = (ref.interpolate64(x, y, w, v, cx + h, cy) - ref.interpolate64(x, y, w, v, cx - h, cy)) / (2 * h) * 2 / W
            dy = (ref.interpolate64(x, y, w, v, cx, cy + h) - ref.interpolate64(x, y, w, v, cx, cy - h)) / (2 * h) * 2 / H
            # binary32 U and barycentrics: a few 1e-7 of the terms' magnitude; the difference quotient: h^2
            tol = 1e-5 * scale[0, iy, ix, a] + 1e-6
            assert abs(deriv[0, iy, ix, a, 0] - dx) <= tol[0], (iy, ix, a, deriv[0, iy, ix, a, 0], dx)
            assert abs(deriv[0, iy, ix, a, 1] - dy) <= tol[1], (iy, ix, a, deriv[0, iy, ix, a, 1], dy)
    if want_constant:
        d = deriv[covered]
        assert np.abs(d - d[0]).max() <= 1e-5 * np.abs(d).max()
    return len(pick)


def test_derivatives_of_a_fronto_parallel_triangle_are_constant():
    clip = np.array([[-0.8, -0.7, 0.2, 1.0], [0.9, -0.5, 0.2, 1.0], [0.1, 0.8, 0.2, 1.0]], np.float32)
    attributes = np.array([[0.0, 1.0], [1.0, 0.25], [0.5, -2.0]], np.float32)
    for order in ([0, 1, 2], [0, 2, 1]):                       # either sign of the adjugate
        triangles = np.array([order], np.int32)
        assert _check_against_central_differences(clip, triangles, attributes, 32, 24, want_constant=True) > 50


def test_derivatives_of_a_strongly_foreshortened_quad():
    # a floor quad seen at a grazing angle: w runs from 0.5 to 8 over the image
    clip = np.array([[-0.5, -0.9, 0.1, 0.5], [0.5, -0.9, 0.1, 0.5], [7.0, 2.0, 0.9, 8.0], [-7.0, 2.0, 0.9, 8.0]],
                    np.float32)
    triangles = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    attributes = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [1.0, 16.0, 1.0], [0.0, 16.0, 1.0]], np.float32)
    assert _check_against_central_differences(clip, triangles, attributes, 40, 30) > 100


def test_derivatives_with_a_vertex_behind_the_camera():
    data = golden_npz("clip_camera_inside_cube.npz")
    clip, triangles = data["clip"], data["triangles"]
    behind = (clip[triangles][..., 3] < 0).any(1)
    assert behind.any()
    ids, _, _ = oracle.forward(clip[None], triangles, 160, 120)
    assert np.isin(ids[0], np.nonzero(behind)[0]).any()      # such triangles are drawn
    g = np.random.RandomState(10)
    attributes = g.randn(8, 2).astype(np.float32)
    assert _check_against_central_differences(clip, triangles, attributes, 160, 120) > 100


# ---- interface ---------------------------------------------------------------------------------------------------
def _mip_args():
    args = _tex_args()
    args.update(uv_da=torch.zeros(2, 5, 7, 4), filter_mode=MIP)
    return args


@pytest.mark.parametrize("name, bad, message", [
    ("filter_mode", "nearest", "filter_mode must be 'linear' or 'linear-mipmap-linear'"),
    ("filter_mode", "linear-mipmap-nearest", "filter_mode must be 'linear' or 'linear-mipmap-linear'"),
    ("filter_mode", "linear", "uv_da is only used with filter_mode='linear-mipmap-linear'"),
    ("uv_da", None, "requires uv_da"),
    ("uv_da", torch.zeros(2, 5, 7, 2), "uv_da must be a float32 tensor of shape"),
    ("uv_da", torch.zeros(2, 5, 6, 4), "uv_da must be a float32 tensor of shape"),
    ("uv_da", torch.zeros(2, 5, 7, 2, 2), "uv_da must be a float32 tensor of shape"),
    ("uv_da", torch.zeros(2, 5, 7, 4, dtype=torch.float64), "uv_da must be a float32 tensor of shape"),
    ("uv_da", [0.0] * 4, "uv_da must be a float32 tensor of shape"),
    ("max_mip_level", -1, "max_mip_level must be None or a non-negative integer"),
    ("max_mip_level", 1.0, "max_mip_level must be None or a non-negative integer"),
    ("max_mip_level", True, "max_mip_level must be None or a non-negative integer"),
    ("boundary_mode", "mirror", "boundary_mode must be 'wrap' or 'clamp'"),
    ("uv", torch.zeros(2, 5, 7, 3), r"uv must have shape \[batch_size, height, width, 2\]"),
])
def test_texture_value_errors(name, bad, message):
    args = _mip_args()
    args[name] = bad
    with pytest.raises(ValueError, match=message):
        mesh_renderer.texture_filtered(**args)


def test_texture_max_mip_level_is_checked_in_linear_mode_too():
    args = _tex_args()
    args["max_mip_level"] = -2
    with pytest.raises(ValueError, match="max_mip_level must be None or a non-negative integer"):
        mesh_renderer.texture_filtered(**args)


@pytest.mark.parametrize("name, bad, message", [
    ("filter_mode", "nearest", "filter_mode must be 'linear' or 'linear-mipmap-linear'"),
    ("filter_mode", None, "filter_mode must be 'linear' or 'linear-mipmap-linear'"),
    ("max_mip_level", -1, "max_mip_level must be None or a non-negative integer"),
    ("max_mip_level", 2.5, "max_mip_level must be None or a non-negative integer"),
])
def test_render_textured_value_errors(name, bad, message):
    args = _render_args()
    args["filter_mode"] = MIP
    args[name] = bad
    with pytest.raises(ValueError, match=message):
        mesh_renderer.render_textured_filtered(**args)


def test_attribute_derivatives_value_errors():
    ids, bary = torch.zeros(2, 6, 8, dtype=torch.int32), torch.zeros(2, 6, 8, 3)
    clip, triangles = torch.zeros(2, 5, 4), torch.zeros(3, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"clip_vertices must have shape \[batch_size, vertex_count, 4\]"):
        mesh_renderer.attribute_derivatives(ids, bary, clip[..., :3], triangles, torch.zeros(5, 2))
    with pytest.raises(ValueError, match="with 1 <= A <= 4"):
        mesh_renderer.attribute_derivatives(ids, bary, clip, triangles, torch.zeros(5, 5))
    with pytest.raises(ValueError, match="one row per vertex when attribute_triangles is None"):
        mesh_renderer.attribute_derivatives(ids, bary, clip, triangles, torch.zeros(6, 2))
    with pytest.raises(ValueError, match="attribute_triangles must have shape"):
        mesh_renderer.attribute_derivatives(ids, bary, clip, triangles, torch.zeros(9, 2),
                                            torch.zeros(4, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="attribute_triangles must be int32"):
        mesh_renderer.attribute_derivatives(ids, bary, clip, triangles, torch.zeros(9, 2), torch.zeros(3, 3))
    with pytest.raises(ValueError, match="barycentrics must have shape"):
        mesh_renderer.attribute_derivatives(ids, bary[:, :5], clip, triangles, torch.zeros(5, 2))


def test_on_the_host_there_is_no_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_renderer.texture_filtered(**_mip_args())
    args = _render_args()
    args["filter_mode"] = MIP
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_renderer.render_textured_filtered(**args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_renderer.attribute_derivatives(torch.zeros(2, 6, 8, dtype=torch.int32), torch.zeros(2, 6, 8, 3),
                                            torch.zeros(2, 5, 4), torch.zeros(3, 3, dtype=torch.int32), torch.zeros(5, 2))
    tex, uv, da = torch.zeros(4, 6, 3), torch.zeros(2, 5, 7, 2), torch.zeros(2, 5, 7, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.texture_mip_forward(tex, uv, da)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.texture_mip_backward(torch.zeros(2, 5, 7, 3), tex, torch.zeros(24), uv, da)
    with pytest.raises(RuntimeError, match="uv_da must be float32"):
        _native.texture_mip_forward(tex, uv, da.double())
    with pytest.raises(ValueError, match="pyramid must have shape"):
        _native.texture_mip_backward(torch.zeros(2, 5, 7, 3), tex, torch.zeros(11), uv, da)


def test_abi_validates_sizes_without_a_gpu():
    L = _native.lib()
    null = ctypes.c_void_p(0)
    assert [L.mr_texture_mip_levels(h, w, m) for h, w, m in ((8, 8, -1), (12, 20, -1), (64, 1, -1), (8, 8, 1),
                                                              (65536, 65536, -1))] == [4, 3, 1, 2, 17]
    assert [L.mr_texture_mip_levels(h, w, -1) for h, w in ((0, 8), (8, 0), (65537, 2), (-4, 4))] == [0, 0, 0, 0]
    # tex_batched, Ht, Wt, C, B, W, H
    bad = [(2, 4, 4, 3, 1, 8, 8), (0, 0, 4, 3, 1, 8, 8), (0, 4, 0, 3, 1, 8, 8), (0, 4, 4, 0, 1, 8, 8),
           (0, 4, 4, 5, 1, 8, 8), (0, 4, 4, 3, -1, 8, 8), (0, 4, 4, 3, 65536, 8, 8), (0, 4, 4, 3, 1, 0, 8),
           (0, 4, 4, 3, 1, 1 << 16, 1 << 15), (0, 1 << 15, 1 << 14, 3, 1, 8, 8), (0, 70000, 1, 3, 1, 8, 8),
           (0, 4, 4, 3, 1, 1, 1 << 30)]
    for dims in bad:
        assert L.mr_texture_mip_backward_workspace_bytes(*dims, -1) == 0
        assert L.mr_texture_mip_forward(null, null, null, null, *dims, 0, -1, null, null, null) == _native.MR_EINVAL
        assert L.mr_texture_mip_backward(null, null, null, null, null, null, *dims, 0, -1, null, null, null, 0,
                                         null) == _native.MR_EINVAL
    ok = (0, 4, 4, 3, 1, 8, 8)
    p16, p4 = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    for boundary in (-1, 2):
        assert L.mr_texture_mip_forward(p16, p16, p16, null, *ok, boundary, -1, p16, p16, null) == _native.MR_EINVAL
    # missing or misaligned buffers are refused before anything is launched; the pyramid only when it has levels
    assert L.mr_texture_mip_forward(null, null, null, null, *ok, 0, -1, null, null, null) == _native.MR_EINVAL
    assert L.mr_texture_mip_forward(p16, p16, null, null, *ok, 0, -1, p16, p16, null) == _native.MR_EINVAL
    assert L.mr_texture_mip_forward(p16, p16, p4, null, *ok, 0, -1, p16, p16, null) == _native.MR_EINVAL
    assert L.mr_texture_mip_forward(p16, p16, p16, null, *ok, 0, -1, null, p16, null) == _native.MR_EINVAL
    assert L.mr_texture_mip_forward(p16, p16, p16, null, *ok, 0, -1, p4, p16, null) == _native.MR_EINVAL
    assert L.mr_texture_mip_backward(p16, p16, null, p16, p16, null, *ok, 0, -1, p16, null, null, 0,
                                     null) == _native.MR_EINVAL
    assert L.mr_texture_mip_backward(p16, p16, p16, p16, p16, null, *ok, 0, -1, p4, null, null, 0,
                                     null) == _native.MR_EINVAL
    # a wanted dtex without the workspace is refused before the launch (the gradient pyramid lives there)
    assert L.mr_texture_mip_backward(p16, p16, p16, p16, p16, null, *ok, 0, -1, p16, null, null, 0,
                                     null) == _native.MR_EWORKSPACE
    # an empty batch is a no-op
    assert L.mr_texture_mip_forward(null, null, null, null, 0, 4, 4, 3, 0, 8, 8, 0, -1, null, null, null) == _native.MR_OK
    assert L.mr_texture_mip_backward(null, null, null, null, null, null, 0, 4, 4, 3, 0, 8, 8, 0, -1, null, null, null, 0,
                                     null) == _native.MR_OK
    # sizes: the pyramid is a third of the texture (rounded up to 4 texels per texture), one per image when batched
    assert L.mr_texture_mip_pyramid_bytes(0, 64, 32, 3, 4, -1) == (512 + 128 + 32 + 8 + 2 + 2) * 3 * 4
    assert L.mr_texture_mip_pyramid_bytes(1, 64, 32, 3, 4, -1) == 4 * (512 + 128 + 32 + 8 + 2 + 2) * 3 * 4
    assert L.mr_texture_mip_pyramid_bytes(0, 64, 32, 3, 4, 1) == 512 * 3 * 4
    assert L.mr_texture_mip_pyramid_bytes(0, 5, 7, 3, 4, -1) == 0
    before = L.mr_set_deterministic(0)
    try:
        need = L.mr_texture_mip_backward_workspace_bytes(0, 64, 32, 3, 4, 8, 8, -1)
        assert need >= 684 * 3 * 4 and need % 256 == 0
        assert L.mr_texture_mip_backward_workspace_bytes(0, 5, 7, 3, 4, 8, 8, -1) == 0
        L.mr_set_deterministic(1)
        need = L.mr_texture_mip_backward_workspace_bytes(0, 64, 32, 3, 4, 8, 8, -1)
        assert need >= (64 * 32 + 682) * 3 * 8 and need % 256 == 0
        assert L.mr_texture_mip_backward_workspace_bytes(1, 64, 32, 3, 4, 8, 8, -1) >= 4 * (64 * 32 + 682) * 3 * 8
    finally:
        L.mr_set_deterministic(before)
    # mr_attribute_derivatives: ids, bary, clip, triangles, attributes, attribute_triangles, B V T Va W H A, out, stream
    for dims in ((1, 8, 12, 8, 16, 16, 0), (1, 8, 12, 8, 16, 16, 5), (1, 8, 0, 8, 16, 16, 2), (1, 0, 12, 8, 16, 16, 2),
                 (1, 8, 12, 0, 16, 16, 2), (-1, 8, 12, 8, 16, 16, 2), (1, 8, 12, 8, 0, 16, 2), (65536, 8, 12, 8, 16, 16, 2)):
        assert L.mr_attribute_derivatives(p16, p16, p16, p16, p16, null, *dims, p16, null) == _native.MR_EINVAL
    good = (1, 8, 12, 8, 16, 16, 2)
    assert L.mr_attribute_derivatives(null, p16, p16, p16, p16, null, *good, p16, null) == _native.MR_EINVAL
    assert L.mr_attribute_derivatives(p16, p16, p4, p16, p16, null, *good, p16, null) == _native.MR_EINVAL
    assert L.mr_attribute_derivatives(p16, p16, p16, p16, p16, null, *good, p4, null) == _native.MR_EINVAL
    assert L.mr_attribute_derivatives(null, null, null, null, null, null, 0, 8, 12, 8, 16, 16, 2, null, null) == _native.MR_OK


def test_new_symbols_are_exported():
    assert mesh_renderer.attribute_derivatives is texturing.attribute_derivatives
    assert mesh_renderer.texture_mip_levels is texturing.texture_mip_levels
    assert issubclass(texturing.TextureMipSample, torch.autograd.Function)
    for name in ("texture_mip_forward", "texture_mip_backward", "texture_mip_pyramid", "texture_mip_levels",
                 "attribute_derivatives"):
        assert callable(getattr(_native, name)), name
    assert mesh_renderer.texture_filtered is texturing.texture_filtered
    assert mesh_renderer.render_textured_filtered is texturing.render_textured_filtered
    # texture() and render_textured() keep their signatures; the *_filtered pair appends the filter arguments to them
    plain = inspect.signature(mesh_renderer.texture).parameters
    params = inspect.signature(mesh_renderer.texture_filtered).parameters
    assert list(params) == list(plain) + ["uv_da", "filter_mode", "max_mip_level"]
    assert [params[k].default for k in plain] == [plain[k].default for k in plain]
    assert [params[k].default for k in list(params)[-3:]] == [None, "linear", None]
    plain = inspect.signature(mesh_renderer.render_textured).parameters
    params = inspect.signature(mesh_renderer.render_textured_filtered).parameters
    assert list(params) == list(plain) + ["filter_mode", "max_mip_level"]
    assert [params[k].default for k in plain] == [plain[k].default for k in plain]
    assert [params[k].default for k in list(params)[-2:]] == ["linear", None]
    assert list(inspect.signature(mesh_renderer.attribute_derivatives).parameters) == [
        "ids", "bary", "clip_vertices", "triangles", "attributes", "attribute_triangles"]
    L = _native.lib()
    for name in ("mr_texture_mip_levels", "mr_texture_mip_pyramid_bytes", "mr_texture_mip_forward",
                 "mr_texture_mip_backward_workspace_bytes", "mr_texture_mip_backward", "mr_attribute_derivatives"):
        assert getattr(L, name).argtypes is not None
    assert "uv_da" in mesh_renderer.texture_filtered.__doc__ and "no gradient" in mesh_renderer.texture_filtered.__doc__
