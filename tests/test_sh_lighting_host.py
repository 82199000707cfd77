"""Spherical-harmonics lighting on the host: the restatement's basis, the package's torch restatement against it, and
the argument checks of sh_shader / render_sh / the _native wrappers and the C ABI (no GPU needed)."""
import ctypes
import importlib
import inspect

import numpy as np
import pytest
import torch

import sh_reference as ref
from pytorch_mesh_renderer_amd import _native, mesh_renderer

sh_lighting = importlib.import_module("pytorch_mesh_renderer_amd.mesh_renderer.sh_lighting")


def test_restatement_basis_is_orthonormal_on_the_sphere():
    pts, weights = ref.sphere_quadrature()
    assert abs(weights.sum() - 4.0 * np.pi) < 1e-12
    Y = ref.basis(pts)                                   # [N, 9]
    gram = (Y * weights[:, None]).T @ Y
    np.testing.assert_allclose(gram, np.eye(9), atol=1e-12)


def test_constant_term_alone_gives_a_uniform_irradiance():
    g = torch.Generator().manual_seed(0)
    normals = torch.randn(2, 5, 7, 3, generator=g, dtype=torch.float64)
    normals[0, 0, 0] = 0.0                               # a zero-length normal as well
    diffuse = torch.ones(2, 5, 7, 3, dtype=torch.float64)
    sh = torch.zeros(2, 9, 3, dtype=torch.float64)
    sh[:, 0, :] = torch.tensor([[0.5, 1.0, 2.0], [3.0, -1.0, 0.25]], dtype=torch.float64)
    rgba = ref.shade(normals, diffuse, None, sh, flip=False)
    want = (0.282094791773878 * sh[:, 0, :])[:, None, None, :].expand(2, 5, 7, 3)
    torch.testing.assert_close(rgba[..., :3], want, rtol=0, atol=1e-15)
    assert bool((rgba[..., 3] == 1).all())


def _buffers(seed, B=2, H=5, W=7):
    g = torch.Generator().manual_seed(seed)
    normals = torch.randn(B, H, W, 3, generator=g)
    normals[:, 0, 0] = 0.0
    diffuse = torch.rand(B, H, W, 3, generator=g)
    diffuse[:, 1] = -1.0                                 # background rows
    alphas = torch.tensor([0.0, 0.3, 0.5, 0.7, 1.0])[torch.randint(0, 5, (B, H, W), generator=g)]
    sh = torch.randn(B, 9, 3, generator=g)
    return normals, alphas, diffuse, sh


@pytest.mark.parametrize("with_alphas", [False, True])
def test_torch_path_matches_the_restatement(monkeypatch, with_alphas):
    monkeypatch.setattr(sh_lighting, "USE_SH_KERNELS", False)
    normals, alphas, diffuse, sh = _buffers(1)
    alphas = alphas if with_alphas else None
    leaves = [normals.clone().requires_grad_(True), diffuse.clone().requires_grad_(True),
              sh.clone().requires_grad_(True)]
    a = alphas.clone().requires_grad_(True) if with_alphas else None
    out = mesh_renderer.sh_shader(leaves[0], a, leaves[1], leaves[2])
    drgba = torch.randn(out.shape, generator=torch.Generator().manual_seed(2))
    (out * drgba).sum().backward()
    want = ref.shade(normals, diffuse, alphas, sh)
    torch.testing.assert_close(out.detach().double(), want, rtol=0, atol=1e-5)
    grads = ref.gradients(normals, diffuse, alphas, sh, drgba)
    for name, leaf in zip(("normals", "diffuse", "sh"), leaves):
        torch.testing.assert_close(leaf.grad.double(), grads[name], rtol=1e-5, atol=1e-5)
    if with_alphas:
        torch.testing.assert_close(a.grad.double(), torch.flip(drgba, [1])[..., 3].double())


def test_torch_path_broadcasts_a_single_set_of_coefficients(monkeypatch):
    monkeypatch.setattr(sh_lighting, "USE_SH_KERNELS", False)
    normals, alphas, diffuse, sh = _buffers(3)
    shared = sh[0].clone().requires_grad_(True)
    out = mesh_renderer.sh_shader(normals, alphas, diffuse, shared)
    torch.testing.assert_close(out, mesh_renderer.sh_shader(normals, alphas, diffuse, sh[0].expand(2, 9, 3)))
    out.sum().backward()
    assert shared.grad.shape == (9, 3)


def _valid_shader_args():
    normals, alphas, diffuse, sh = _buffers(4)
    return {"normals": normals, "alphas": alphas, "diffuse_colors": diffuse, "sh_coefficients": sh}


@pytest.mark.parametrize("name, bad, message", [
    ("normals", torch.zeros(2, 5, 7), "normals must have shape"),
    ("normals", torch.zeros(2, 5, 7, 4), "normals must have shape"),
    ("diffuse_colors", torch.zeros(2, 5, 6, 3), "diffuse_colors must have shape"),
    ("alphas", torch.zeros(2, 5, 7, 1), "alphas must have shape"),
    ("sh_coefficients", torch.zeros(2, 9, 4), r"must have shape \[batch_size, 9, 3\] or \[9, 3\]"),
    ("sh_coefficients", torch.zeros(3, 9, 3), r"must have shape \[batch_size, 9, 3\] or \[9, 3\]"),
    ("sh_coefficients", torch.zeros(27), r"must have shape \[batch_size, 9, 3\] or \[9, 3\]"),
])
def test_sh_shader_value_errors(name, bad, message):
    args = _valid_shader_args()
    args[name] = bad
    with pytest.raises(ValueError, match=message):
        mesh_renderer.sh_shader(**args)


def test_sh_shader_on_the_host_has_no_fallback():
    assert sh_lighting.USE_SH_KERNELS is True
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_renderer.sh_shader(**_valid_shader_args())
    args = _valid_shader_args()
    args["alphas"] = None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_renderer.sh_shader(**args)


def _valid_render_args():
    return {"vertices": torch.zeros(2, 8, 3), "triangles": torch.zeros(12, 3, dtype=torch.int32),
            "normals": torch.zeros(2, 8, 3), "diffuse_colors": torch.zeros(2, 8, 3),
            "sh_coefficients": torch.zeros(9, 3), "camera_position": torch.tensor([0.0, 0.0, 5.0]),
            "camera_lookat": torch.zeros(3), "camera_up": torch.tensor([0.0, 1.0, 0.0]),
            "image_width": 16, "image_height": 12}


@pytest.mark.parametrize("name, bad, message", [
    ("vertices", torch.zeros(2, 8), r"Vertices must have shape \[batch_size, vertex_count, 3\]"),
    ("normals", torch.zeros(2, 8, 4), r"Normals must have shape \[batch_size, vertex_count, 3\]"),
    ("diffuse_colors", torch.zeros(2, 8), r"diffuse_colors must have shape \[batch_size, vertex_count, 3\]"),
    ("sh_coefficients", torch.zeros(1, 9, 3), r"sh_coefficients must have shape \[batch_size, 9, 3\] or \[9, 3\]"),
    ("sh_coefficients", torch.zeros(9, 2), r"sh_coefficients must have shape \[batch_size, 9, 3\] or \[9, 3\]"),
    ("camera_position", torch.zeros(3, 3), r"camera_position must have shape \[batch_size, 3\] or \[3\]"),
    ("camera_lookat", torch.zeros(2), r"camera_lookat must have shape \[batch_size, 3\] or \[3\]"),
    ("camera_up", torch.zeros(2, 2), r"camera_up must have shape \[batch_size, 3\] or \[3\]"),
    ("fov_y", torch.zeros(3), "fov_y must be a float, a 0D tensor, or a 1D tensor"),
])
def test_render_sh_value_errors(name, bad, message):
    args = _valid_render_args()
    args[name] = bad
    with pytest.raises(ValueError, match=message):
        mesh_renderer.render_sh(**args)


def test_native_wrappers_check_dtypes_shapes_and_device():
    normals, alphas, diffuse, sh = _buffers(5)
    drgba = torch.zeros(2, 5, 7, 4)
    with pytest.raises(RuntimeError, match="normals must be float32"):
        _native.sh_shade_forward(normals.double(), diffuse, alphas, sh)
    with pytest.raises(RuntimeError, match="alphas must be float32"):
        _native.sh_shade_forward(normals, diffuse, alphas.half(), sh)
    with pytest.raises(RuntimeError, match="sh coefficients must be float32"):
        _native.sh_shade_backward(drgba, normals, diffuse, alphas, sh.double())
    with pytest.raises(ValueError, match="diffuse colors must have shape"):
        _native.sh_shade_forward(normals, diffuse[:, :4], alphas, sh)
    with pytest.raises(ValueError, match="sh coefficients must have shape"):
        _native.sh_shade_forward(normals, diffuse, alphas, sh[0])
    with pytest.raises(ValueError, match="upstream gradient must have shape"):
        _native.sh_shade_backward(drgba[..., :3], normals, diffuse, alphas, sh)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.sh_shade_forward(normals, diffuse, alphas, sh)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.sh_shade_backward(drgba, normals, diffuse, None, sh)


def test_packed_channel_slices_are_read_in_place():
    packed = torch.zeros(2, 5, 7, 6)
    assert _native._pixel_stride(packed[..., 0:3], packed[..., 3:6]) == (6, 0, 3)
    wide = torch.zeros(2, 5, 7, 9)
    assert _native._pixel_stride(wide[..., 6:9], wide[..., 0:3]) == (9, 6, 0)
    assert _native._pixel_stride(packed[..., 0:3], packed[..., 1:4]) is None          # overlapping channels
    assert _native._pixel_stride(packed[..., 0:3], torch.zeros(2, 5, 7, 6)[..., 3:6]) is None   # two buffers
    assert _native._pixel_stride(packed[:, :, 1:, 0:3], packed[:, :, 1:, 3:6]) is None   # not whole rows
    assert _native._pixel_stride(torch.zeros(2, 5, 7, 3), torch.zeros(2, 5, 7, 3)) is None


def test_abi_validates_sizes_without_a_gpu():
    L = _native.lib()
    null = ctypes.c_void_p(0)
    assert L.mr_sh_shade_backward_workspace_bytes(1, 0, 4) == 0
    assert L.mr_sh_shade_backward_workspace_bytes(-1, 4, 4) == 0
    assert L.mr_sh_shade_backward_workspace_bytes(70000, 4, 4) == 0
    assert L.mr_sh_shade_backward_workspace_bytes(1, 1 << 16, 1 << 15) == 0
    need = L.mr_sh_shade_backward_workspace_bytes(32, 1024, 1024)
    assert need >= 32 * 1024 * 27 * 4 and need % 256 == 0
    for B, W, H, stride in ((1, 0, 4, 3), (-1, 4, 4, 3), (1, 4, 4, 2), (65536, 4, 4, 3)):
        assert L.mr_sh_shade_forward(null, null, stride, null, null, B, W, H, 1, null, null) == _native.MR_EINVAL
        assert L.mr_sh_shade_backward(null, null, null, stride, null, null, B, W, H, 1, null, null, null, null,
                                      null, 0, null) == _native.MR_EINVAL
    # missing buffers are refused before anything is launched
    assert L.mr_sh_shade_forward(null, null, 3, null, null, 1, 4, 4, 1, null, null) == _native.MR_EINVAL
    assert L.mr_sh_shade_backward(null, null, null, 3, null, null, 1, 4, 4, 1, null, null, null, null,
                                  null, 0, null) == _native.MR_EINVAL
    # an empty batch is a no-op
    assert L.mr_sh_shade_forward(null, null, 3, null, null, 0, 4, 4, 1, null, null) == _native.MR_OK


def test_new_symbols_are_exported():
    assert mesh_renderer.sh_shader is sh_lighting.sh_shader
    assert mesh_renderer.render_sh is sh_lighting.render_sh
    assert issubclass(sh_lighting.SHShade, torch.autograd.Function)
    assert issubclass(sh_lighting.SHShadePacked, torch.autograd.Function)
    assert _native.ABI_VERSION == 356 and _native.lib().mr_version() == 356
    params = list(inspect.signature(mesh_renderer.render_sh).parameters)
    assert params == ["vertices", "triangles", "normals", "diffuse_colors", "sh_coefficients", "camera_position",
                      "camera_lookat", "camera_up", "image_width", "image_height", "fov_y", "near_clip", "far_clip",
                      "antialias"]
    assert list(inspect.signature(mesh_renderer.sh_shader).parameters) == [
        "normals", "alphas", "diffuse_colors", "sh_coefficients"]


def test_render_signature_is_unchanged():
    params = inspect.signature(mesh_renderer.render).parameters
    assert list(params) == ["vertices", "triangles", "normals", "diffuse_colors", "camera_position",
                            "camera_lookat", "camera_up", "light_positions", "light_intensities", "image_width",
                            "image_height", "specular_colors", "shininess_coefficients", "ambient_color", "fov_y",
                            "near_clip", "far_clip", "antialias"]
    defaults = {k: p.default for k, p in params.items() if p.default is not inspect.Parameter.empty}
    assert defaults == {"specular_colors": None, "shininess_coefficients": None, "ambient_color": None,
                        "fov_y": 40.0, "near_clip": 0.01, "far_clip": 10.0, "antialias": False}
