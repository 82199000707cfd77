"""Texture mapping on the host: the float64 restatement against torch's grid_sample and against central
differences, sphere_uvs, and the argument checks of texture / render_textured / the _native wrappers and the C ABI
(no GPU needed)."""
import ctypes
import importlib
import inspect
import math

import pytest
import torch

import texture_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from pytorch_mesh_renderer_amd.common import shapes

texturing = importlib.import_module("pytorch_mesh_renderer_amd.mesh_renderer.texturing")
F = torch.nn.functional


def _off_centre_uv(B, H, W, Ht, Wt, lo, hi, seed):
    """UVs whose x = u * Wt - 0.5 (and y) lie in [lo, hi) texels and at least 0.05 texel from an integer, where
    floor() and grid_sample could pick different cells."""
    g = torch.Generator().manual_seed(seed)
    cell = torch.randint(lo, hi, (B, H, W, 2), generator=g).double()
    frac = 0.05 + 0.9 * torch.rand(B, H, W, 2, generator=g, dtype=torch.float64)
    xy = cell + frac
    return torch.stack([(xy[..., 0] + 0.5) / Wt, (xy[..., 1] + 0.5) / Ht], 3)


def _grid_sample(tex, uv, boundary):
    """The same lookup through grid_sample(align_corners=False): border padding for clamp; for wrap the texture
    padded circularly by one texel and sampled at frac(u)."""
    B = uv.shape[0]
    t = tex if tex.dim() == 4 else tex.unsqueeze(0).expand(B, *tex.shape)
    t = t.permute(0, 3, 1, 2)
    Ht, Wt = t.shape[2], t.shape[3]
    if boundary == "clamp":
        return F.grid_sample(t, 2.0 * uv - 1.0, mode="bilinear", padding_mode="border",
                             align_corners=False).permute(0, 2, 3, 1)
    tp = F.pad(t, (1, 1, 1, 1), mode="circular")
    f = uv - torch.floor(uv)
    up = (f[..., 0] * Wt + 1.0) / (Wt + 2)
    vp = (f[..., 1] * Ht + 1.0) / (Ht + 2)
    grid = 2.0 * torch.stack([up, vp], 3) - 1.0
    return F.grid_sample(tp, grid, mode="bilinear", padding_mode="zeros", align_corners=False).permute(0, 2, 3, 1)


@pytest.mark.parametrize("boundary", ["wrap", "clamp"])
@pytest.mark.parametrize("batched", [False, True])
def test_reference_matches_grid_sample(boundary, batched):
    B, H, W, Ht, Wt, C = 3, 5, 6, 7, 11, 3
    g = torch.Generator().manual_seed(1)
    tex = torch.randn(*((B,) if batched else ()), Ht, Wt, C, generator=g, dtype=torch.float64)
    uv = _off_centre_uv(B, H, W, Ht, Wt, -3 * max(Ht, Wt), 3 * max(Ht, Wt), 2)
    dout = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    value, dtex, duv, _ = ref.sample(tex, uv, None, boundary, dout)
    t_leaf, uv_leaf = tex.clone().requires_grad_(True), uv.clone().requires_grad_(True)
    want = _grid_sample(t_leaf, uv_leaf, boundary)
    (want * dout).sum().backward()
    # the restatement rounds x and y to binary32 (|x| < 40 here: fx within 2^-18 of grid_sample's float64)
    torch.testing.assert_close(value, want.detach(), rtol=0, atol=2e-5)
    torch.testing.assert_close(dtex, t_leaf.grad, rtol=0, atol=2e-5)
    torch.testing.assert_close(duv, uv_leaf.grad, rtol=0, atol=2e-5 * max(Ht, Wt))


def test_reference_gradients_match_central_differences():
    B, H, W, Ht, Wt, C = 2, 3, 4, 5, 9, 2
    g = torch.Generator().manual_seed(3)
    tex = torch.randn(Ht, Wt, C, generator=g, dtype=torch.float64)
    uv = _off_centre_uv(B, H, W, Ht, Wt, -2 * Wt, 2 * Wt, 4)
    dout = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    for boundary in ("wrap", "clamp"):
        _, dtex, duv, _ = ref.sample(tex, uv, None, boundary, dout)

        def loss(t, q):
            return float((ref.sample(t, q, None, boundary) * dout).sum())
        # the value is linear in the texture: one texel's difference quotient is exact
        for (i, j, c) in ((0, 0, 0), (2, 5, 1), (4, 8, 0)):
            e = torch.zeros_like(tex)
            e[i, j, c] = 1.0
            fd = (loss(tex + e, uv) - loss(tex - e, uv)) / 2.0
            assert abs(fd - float(dtex[i, j, c])) < 1e-9
        # in u (or v) alone it is linear inside a cell, so a step of 0.04 texel, which stays inside (>= 0.05 texel
        # from a cell edge), is exact but for the binary32 rounding of x (~2^-20 texel here)
        h = 0.04 / max(Ht, Wt)
        for k in range(2):
            for idx in ((0, 0, 0), (1, 2, 3), (0, 1, 2)):
                d = torch.zeros_like(uv)
                d[idx + (k,)] = h
                fd = (float((ref.sample(tex, uv + d, None, boundary) * dout)[idx].sum())
                      - float((ref.sample(tex, uv - d, None, boundary) * dout)[idx].sum())) / (2 * h)
                assert abs(fd - float(duv[idx + (k,)])) < 1e-4 * max(1.0, abs(fd)), (boundary, k, idx)


def test_reference_skips_masked_non_finite_and_huge_coordinates():
    tex = torch.arange(1.0, 13.0, dtype=torch.float64).view(2, 2, 3)
    uv = torch.full((1, 1, 6, 2), 0.3, dtype=torch.float64)
    uv[0, 0, 1, 0] = float("nan")
    uv[0, 0, 2, 1] = float("inf")
    uv[0, 0, 3, 0] = 2.0 ** 23 + 1.0         # x = u * 2 - 0.5 >= 2^24
    mask = torch.ones(1, 1, 6, dtype=torch.float64)
    mask[0, 0, 4] = 0.5
    dout = torch.ones(1, 1, 6, 3, dtype=torch.float64)
    value, dtex, duv, _ = ref.sample(tex, uv, mask, "wrap", dout)
    assert bool((value[0, 0, 1:5] == 0).all()) and bool((duv[0, 0, 1:5] == 0).all())
    assert bool((value[0, 0, 0] != 0).all()) and bool((value[0, 0, 5] != 0).all())
    torch.testing.assert_close(dtex.sum(), torch.tensor(6.0, dtype=torch.float64))   # 2 pixels x 3 channels


def test_sphere_uvs_shapes_and_layout():
    vertices, triangles, _ = shapes.sphere(1.0, 50)
    uvs, uv_triangles = shapes.sphere_uvs(50)
    T = triangles.shape[0]
    assert uvs.shape == (3 * T, 2) and uvs.dtype == torch.float32
    assert uv_triangles.shape == (T, 3) and uv_triangles.dtype == torch.int32
    assert torch.equal(uv_triangles, torch.arange(3 * T, dtype=torch.int32).view(T, 3))


@pytest.mark.parametrize("resolution", [7, 50])
def test_sphere_uvs_are_equirectangular_and_seamless(resolution):
    vertices, triangles, _ = shapes.sphere(1.0, resolution)
    uvs, _ = shapes.sphere_uvs(resolution)
    uv = uvs.double().view(-1, 3, 2)
    p = vertices.double()[triangles.long()]                                   # [T,3,3]
    d = p / p.norm(dim=-1, keepdim=True)
    want_v = 1.0 - torch.acos(d[..., 1].clamp(-1, 1)) / math.pi
    want_u = torch.remainder(torch.atan2(d[..., 0], d[..., 2]) / (2 * math.pi), 1.0)
    pole = d[..., 1].abs() == 1.0
    assert int(pole.sum()) > 0
    torch.testing.assert_close(uv[..., 1], want_v, rtol=0, atol=1e-6)
    du = torch.remainder(uv[..., 0] - want_u + 0.5, 1.0) - 0.5                # modulo 1 in u
    assert float(du[~pole].abs().max()) < 1e-6
    assert float(uv[..., 0].min()) >= 0.0 and float(uv[..., 0].max()) < 1.5
    clean = ~pole.any(1)
    span = uv[..., 0].max(1).values - uv[..., 0].min(1).values
    assert float(span[clean].max()) <= 0.5
    # a pole corner takes the mean u of its triangle's other (non-pole) corners
    t = int(torch.nonzero(pole.sum(1) == 1)[0])
    k = int(torch.nonzero(pole[t])[0])
    others = [i for i in range(3) if i != k]
    assert abs(float(uv[t, k, 0]) - float(uv[t, others, 0].mean())) < 1e-6


def _tex_args():
    return {"tex": torch.zeros(4, 6, 3), "uv": torch.zeros(2, 5, 7, 2), "mask": torch.ones(2, 5, 7),
            "boundary_mode": "wrap"}


@pytest.mark.parametrize("name, bad, message", [
    ("uv", torch.zeros(2, 5, 7), r"uv must have shape \[batch_size, height, width, 2\]"),
    ("uv", torch.zeros(2, 5, 7, 3), r"uv must have shape \[batch_size, height, width, 2\]"),
    ("uv", torch.zeros(2, 5, 7, 2, dtype=torch.float64), "tex and uv must be float32"),
    ("tex", torch.zeros(4, 6), r"tex must have shape \[Ht, Wt, C\] or \[batch_size, Ht, Wt, C\]"),
    ("tex", torch.zeros(3, 4, 6, 3), r"tex must have shape \[Ht, Wt, C\] or \[batch_size, Ht, Wt, C\]"),
    ("tex", torch.zeros(4, 6, 5), "tex must have 1 to 4 channels"),
    ("tex", torch.zeros(4, 6, 0), "tex must have 1 to 4 channels"),
    ("tex", torch.zeros(0, 6, 3), "at least one texel"),
    ("tex", torch.zeros(4, 6, 3, dtype=torch.float16), "tex and uv must be float32"),
    ("mask", torch.ones(2, 5, 6), "mask must be a float32 tensor of shape"),
    ("mask", torch.ones(2, 5, 7, dtype=torch.bool), "mask must be a float32 tensor of shape"),
    ("boundary_mode", "mirror", "boundary_mode must be 'wrap' or 'clamp'"),
])
def test_texture_value_errors(name, bad, message):
    args = _tex_args()
    args[name] = bad
    with pytest.raises(ValueError, match=message):
        mesh_renderer.texture(**args)


def test_texture_on_the_host_has_no_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_renderer.texture(**_tex_args())
    args = _tex_args()
    args["mask"] = None
    args["tex"] = torch.zeros(2, 4, 6, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_renderer.texture(**args)


def _render_args():
    return {"vertices": torch.zeros(2, 8, 3), "triangles": torch.zeros(12, 3, dtype=torch.int32),
            "uvs": torch.zeros(8, 2), "texture": torch.zeros(4, 4, 3),
            "camera_position": torch.tensor([0.0, 0.0, 5.0]), "camera_lookat": torch.zeros(3),
            "camera_up": torch.tensor([0.0, 1.0, 0.0]), "image_width": 16, "image_height": 12}


@pytest.mark.parametrize("name, bad, message", [
    ("vertices", torch.zeros(2, 8), r"Vertices must have shape \[batch_size, vertex_count, 3\]"),
    ("triangles", torch.zeros(12, 4, dtype=torch.int32), r"Triangles must have shape \[triangle_count, 3\]"),
    ("uvs", torch.zeros(8, 3), r"uvs must have shape \[uv_count, 2\] or \[batch_size, uv_count, 2\]"),
    ("uvs", torch.zeros(3, 8, 2), r"uvs must have shape \[uv_count, 2\] or \[batch_size, uv_count, 2\]"),
    ("uvs", torch.zeros(9, 2), "uvs must have one row per vertex when uv_triangles is None"),
    ("uv_triangles", torch.zeros(11, 3, dtype=torch.int32), r"uv_triangles must have shape \[triangle_count, 3\]"),
    ("uv_triangles", torch.zeros(12, 3, dtype=torch.int64), "uv_triangles must be int32"),
    ("texture", torch.zeros(4, 4, 4), "texture must have 3 channels"),
    ("texture", torch.zeros(4, 4, 1), "texture must have 3 channels"),
    ("texture", torch.zeros(3, 4, 4, 3), r"texture must have shape \[Ht, Wt, 3\] or \[batch_size, Ht, Wt, 3\]"),
    ("sh_coefficients", torch.zeros(9, 3), "normals are required with sh_coefficients"),
    ("boundary_mode", "repeat", "boundary_mode must be 'wrap' or 'clamp'"),
    ("camera_position", torch.zeros(3, 3), r"camera_position must have shape \[batch_size, 3\] or \[3\]"),
    ("camera_up", torch.zeros(2, 2), r"camera_up must have shape \[batch_size, 3\] or \[3\]"),
    ("fov_y", torch.zeros(3), "fov_y must be a float, a 0D tensor, or a 1D tensor"),
])
def test_render_textured_value_errors(name, bad, message):
    args = _render_args()
    args[name] = bad
    with pytest.raises(ValueError, match=message):
        mesh_renderer.render_textured(**args)


def test_render_textured_refuses_indices_the_kernels_would_read_out_of_bounds():
    args = _render_args()
    args["normals"], args["sh_coefficients"] = torch.zeros(2, 7, 3), torch.zeros(9, 3)   # V' = 7 < V = 8
    with pytest.raises(ValueError, match=r"Normals must have shape \[batch_size, vertex_count, 3\]"):
        mesh_renderer.render_textured(**args)
    for bad in (12, -1):
        args = _render_args()
        args["uvs"] = torch.zeros(12, 2)
        args["uv_triangles"] = torch.arange(36, dtype=torch.int32).view(12, 3) % 12
        args["uv_triangles"][5, 1] = bad
        with pytest.raises(ValueError, match="uv_triangles must index rows of uvs"):
            mesh_renderer.render_textured(**args)


def test_render_textured_sh_errors_use_render_sh_messages():
    args = _render_args()
    args["normals"] = torch.zeros(2, 8, 3)
    args["sh_coefficients"] = torch.zeros(9, 2)
    with pytest.raises(ValueError, match=r"sh_coefficients must have shape \[batch_size, 9, 3\] or \[9, 3\]"):
        mesh_renderer.render_textured(**args)
    args["sh_coefficients"] = torch.zeros(9, 3)
    args["normals"] = torch.zeros(2, 8, 4)
    with pytest.raises(ValueError, match=r"Normals must have shape \[batch_size, vertex_count, 3\]"):
        mesh_renderer.render_textured(**args)


def test_render_textured_on_the_host_has_no_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_renderer.render_textured(**_render_args())


def test_native_wrappers_check_dtypes_shapes_and_device():
    tex, uv, mask = torch.zeros(4, 6, 3), torch.zeros(2, 5, 7, 2), torch.ones(2, 5, 7)
    dout = torch.zeros(2, 5, 7, 3)
    with pytest.raises(RuntimeError, match="texture must be float32"):
        _native.texture_forward(tex.double(), uv, mask)
    with pytest.raises(RuntimeError, match="uv must be float32"):
        _native.texture_forward(tex, uv.half(), mask)
    with pytest.raises(RuntimeError, match="mask must be float32"):
        _native.texture_backward(dout, tex, uv, mask.double())
    with pytest.raises(ValueError, match="mask must have shape"):
        _native.texture_forward(tex, uv, mask[:, :4])
    with pytest.raises(ValueError, match="texture must have shape"):
        _native.texture_forward(torch.zeros(3, 4, 6, 3), uv, mask)
    with pytest.raises(ValueError, match="1 to 4 channels"):
        _native.texture_forward(torch.zeros(4, 6, 5), uv, mask)
    with pytest.raises(ValueError, match="boundary_mode"):
        _native.texture_forward(tex, uv, mask, "mirror")
    with pytest.raises(ValueError, match="upstream gradient must have shape"):
        _native.texture_backward(dout[..., :2], tex, uv, mask)
    thin = torch.zeros(1).expand(1, 1 << 27, 1, 2)           # 2^27 pixels in one column: 2^23 tiles of 64 x 16
    with pytest.raises(ValueError, match="2\\^22 tiles"):
        _native.texture_forward(tex, thin)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.texture_forward(tex, uv, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.texture_backward(dout, tex, uv, None)


def test_abi_validates_sizes_without_a_gpu():
    L = _native.lib()
    null = ctypes.c_void_p(0)
    # tex_batched, Ht, Wt, C, B, W, H
    bad = [(2, 4, 4, 3, 1, 8, 8), (0, 0, 4, 3, 1, 8, 8), (0, 4, 0, 3, 1, 8, 8), (0, 4, 4, 0, 1, 8, 8),
           (0, 4, 4, 5, 1, 8, 8), (0, 4, 4, 3, -1, 8, 8), (0, 4, 4, 3, 65536, 8, 8), (0, 4, 4, 3, 1, 0, 8),
           (0, 4, 4, 3, 1, 1 << 16, 1 << 15), (0, 1 << 15, 1 << 14, 3, 1, 8, 8), (0, 70000, 1, 3, 1, 8, 8),
           (0, 4, 4, 3, 1, 1, 1 << 30), (0, 4, 4, 3, 1, 1 << 30, 1)]     # thin: more than 2^22 tiles of 64 x 16
    for dims in bad:
        assert L.mr_texture_backward_workspace_bytes(*dims) == 0
        assert L.mr_texture_forward(null, null, null, *dims, 0, null, null) == _native.MR_EINVAL
        assert L.mr_texture_backward(null, null, null, null, *dims, 0, null, null, null, 0,
                                     null) == _native.MR_EINVAL
    ok = (0, 4, 4, 3, 1, 8, 8)
    for boundary in (-1, 2):
        assert L.mr_texture_forward(null, null, null, *ok, boundary, null, null) == _native.MR_EINVAL
        assert L.mr_texture_backward(null, null, null, null, *ok, boundary, null, null, null, 0,
                                     null) == _native.MR_EINVAL
    # missing or misaligned buffers are refused before anything is launched
    assert L.mr_texture_forward(null, null, null, *ok, 0, null, null) == _native.MR_EINVAL
    p16, p4 = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    assert L.mr_texture_forward(p4, p16, null, *ok, 0, p16, null) == _native.MR_EINVAL
    assert L.mr_texture_forward(p16, p4, null, *ok, 0, p16, null) == _native.MR_EINVAL
    assert L.mr_texture_backward(null, p16, p16, null, *ok, 0, p16, null, null, 0, null) == _native.MR_EINVAL
    assert L.mr_texture_backward(p16, p16, p16, null, *ok, 0, p4, null, null, 0, null) == _native.MR_EINVAL
    # an empty batch is a no-op
    assert L.mr_texture_forward(null, null, null, 0, 4, 4, 3, 0, 8, 8, 0, null, null) == _native.MR_OK
    assert L.mr_texture_backward(null, null, null, null, 0, 4, 4, 3, 0, 8, 8, 0, null, null, null, 0,
                                 null) == _native.MR_OK
    # the workspace is needed by the deterministic mode only: 64-bit sums of the texture plus a side block
    before = L.mr_set_deterministic(0)
    try:
        assert L.mr_texture_backward_workspace_bytes(0, 64, 32, 3, 4, 8, 8) == 0
        L.mr_set_deterministic(1)
        need = L.mr_texture_backward_workspace_bytes(0, 64, 32, 3, 4, 8, 8)
        assert need >= 64 * 32 * 3 * 8 and need % 256 == 0
        assert L.mr_texture_backward_workspace_bytes(1, 64, 32, 3, 4, 8, 8) >= 4 * 64 * 32 * 3 * 8
        # a wanted dtex without the workspace is refused before the launch
        assert L.mr_texture_backward(p16, p16, p16, null, *ok, 0, p16, null, null, 0,
                                     null) == _native.MR_EWORKSPACE
    finally:
        L.mr_set_deterministic(before)


def test_new_symbols_are_exported():
    assert mesh_renderer.texture is texturing.texture
    assert mesh_renderer.render_textured is texturing.render_textured
    assert issubclass(texturing.TextureSample, torch.autograd.Function)
    assert callable(shapes.sphere_uvs)
    assert _native.ABI_VERSION == 356 and _native.lib().mr_version() == 356
    assert list(inspect.signature(mesh_renderer.texture).parameters) == ["tex", "uv", "mask", "boundary_mode"]
    params = inspect.signature(mesh_renderer.render_textured).parameters
    assert list(params) == ["vertices", "triangles", "uvs", "texture", "camera_position", "camera_lookat",
                            "camera_up", "image_width", "image_height", "uv_triangles", "normals",
                            "sh_coefficients", "fov_y", "near_clip", "far_clip", "boundary_mode", "antialias"]
    defaults = {k: p.default for k, p in params.items() if p.default is not inspect.Parameter.empty}
    assert defaults == {"uv_triangles": None, "normals": None, "sh_coefficients": None, "fov_y": 40.0,
                        "near_clip": 0.01, "far_clip": 10.0, "boundary_mode": "wrap", "antialias": False}
    L = _native.lib()
    for name in ("mr_texture_forward", "mr_texture_backward_workspace_bytes", "mr_texture_backward"):
        assert getattr(L, name).argtypes is not None

