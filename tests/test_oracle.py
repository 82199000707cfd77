"""CPU suite, part 1: the oracle is pinned against the reference.

oracle/mr_oracle.c must reproduce, bit for bit, every golden vector that
tools/make_goldens.py captured from the reference's own kernel, and -- when the
compiled reference (oracle/_ref) is present -- the reference itself on fresh
random inputs.  oracle/shading.py must reproduce the reference's rasterize() /
render() outputs and gradients.
"""
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import shading, truth64
from conftest import (GOLDEN, golden_sphere_job, TRIANGLE_CASES, bits_equal, golden_json, golden_npz, seeded_dbary, sha)
from pytorch_mesh_renderer_amd.common import synthetic


def test_cube64_bitwise():
    g = golden_npz("raster_cube64.npz")
    ids, bary, z = oracle.forward(g["clip"], g["triangles"], 64, 64)
    assert bits_equal(ids, g["ids"]) and bits_equal(bary, g["bary"]) and bits_equal(z, g["z"])
    dclip = oracle.backward(g["dbary"], g["clip"], g["triangles"], ids, bary)
    assert bits_equal(dclip, g["dclip"])
    assert np.all(dclip[:, 2] == 0.0)  # the z column never receives gradient


@pytest.mark.parametrize("case", TRIANGLE_CASES)
def test_triangle_cases_bitwise(case):
    g = golden_npz("raster_triangles_160x120.npz")
    clip, tris = g[case + ".clip"], g[case + ".triangles"]
    ids, bary, z = oracle.forward(clip, tris, 160, 120)
    assert bits_equal(ids, g[case + ".ids"])
    assert bits_equal(bary, g[case + ".bary"])
    assert bits_equal(z, g[case + ".z"])
    dbary = seeded_dbary((120, 160, 3), seed=1).numpy()
    assert bits_equal(oracle.backward(dbary, clip, tris, ids, bary), g[case + ".dclip"])


def test_reference_semantics_in_goldens():
    """Behaviours the survey probed on the reference (no culling, ties, clipping)."""
    g = golden_npz("raster_triangles_160x120.npz")
    covered = lambda c: int((g[c + ".bary"].sum(-1) > 0.5).sum())
    assert covered("w_111") == covered("reversed_winding") > 0        # both windings draw
    assert covered("all_w_negative") == 0 and covered("collinear") == 0
    assert covered("beyond_far_plane") == 0                            # z > 1 rejected
    tie = g["coincident_tie.ids"][g["coincident_tie.bary"].sum(-1) > 0.5]
    assert np.all(tie == 1)                                            # ties -> later id
    assert covered("one_w_negative") > covered("w_111")                # full-screen bbox path


def test_native_resolution_triangles_hashes():
    g = golden_npz("raster_triangles_160x120.npz")
    h = golden_json("raster_triangles_640x480.json")
    for case in ("w_111", "w_perspective"):
        ids, bary, z = oracle.forward(g[case + ".clip"], g[case + ".triangles"], 640, 480)
        assert sha(ids) == h[case]["ids"] and sha(bary) == h[case]["bary"] and sha(z) == h[case]["z"]
        d = oracle.backward(seeded_dbary((480, 640, 3), seed=1).numpy(), g[case + ".clip"],
                            g[case + ".triangles"], ids, bary)
        assert bits_equal(d, np.array(h[case]["dclip"], np.float32))


def test_jacobian_28x21_bitwise():
    g = golden_npz("raster_jacobian_28x21.npz")
    ids, bary, z = oracle.forward(g["clip"], g["triangles"], 28, 21)
    assert bits_equal(ids, g["ids"]) and bits_equal(bary, g["bary"])
    n = 21 * 28 * 3
    for i in range(0, n, 7):  # every 7th column of the Jacobian
        e = np.zeros(n, np.float32)
        e[i] = 1.0
        d = oracle.backward(e.reshape(21, 28, 3), g["clip"], g["triangles"], ids, bary)
        assert bits_equal(d.reshape(-1), g["jacobian"][:, i])


def test_sphere_256_all_cameras():
    h = golden_json("raster_sphere_hashes.json")["c2_256x256_b8"]
    job = golden_sphere_job("sphere_clip_256_b8.npy")
    assert sha(job["clip"].numpy()) == h["clip"]  # same input bits as when the goldens were made
    ids, bary, z = oracle.forward(job["clip"].numpy(), job["triangles"].numpy(), 256, 256, threads=8)
    for b in range(8):
        assert sha(ids[b]) == h["cameras"][b]["ids"]
        assert sha(bary[b]) == h["cameras"][b]["bary"]
        assert sha(z[b]) == h["cameras"][b]["z"]
        d = oracle.backward(seeded_dbary((256, 256, 3), seed=b).numpy(), job["clip"][b].numpy(),
                            job["triangles"].numpy(), ids[b], bary[b])
        assert sha(d) == h["cameras"][b]["dclip"]
    cam0 = golden_npz("raster_sphere256_cam0.npz")
    assert bits_equal(ids[0], cam0["ids"]) and bits_equal(z[0], cam0["z"])


def test_sphere_1024_picked_cameras():
    h = golden_json("raster_sphere_hashes.json")["c3_1024x1024_b32"]
    dgold = golden_npz("raster_sphere1024_dclip.npz")
    job = golden_sphere_job("sphere_clip_1024_b32.npy")
    assert sha(job["clip"].numpy()) == h["clip"]
    for b in (0, 16):
        clip = job["clip"][b].numpy()
        ids, bary, z = oracle.forward(clip, job["triangles"].numpy(), 1024, 1024)
        hb = h["cameras"][str(b)]
        assert sha(ids) == hb["ids"] and sha(bary) == hb["bary"] and sha(z) == hb["z"]
        d = oracle.backward(seeded_dbary((1024, 1024, 3), seed=b).numpy(), clip,
                            job["triangles"].numpy(), ids, bary)
        assert bits_equal(d, dgold["dclip_%d" % b])


@pytest.mark.skipif(not oracle.have_reference_kernel(), reason="oracle/_ref not built")
def test_against_compiled_reference_random():
    """Differential fuzz: random soups, odd sizes, vertices behind the eye."""
    rng = np.random.default_rng(1234)
    for trial in range(12):
        V, T = int(rng.integers(3, 40)), int(rng.integers(1, 60))
        W, H = int(rng.integers(1, 90)), int(rng.integers(1, 70))
        clip = rng.normal(size=(V, 4)).astype(np.float32)
        clip[:, 3] = np.abs(clip[:, 3]) + 0.2 if trial % 3 else clip[:, 3]  # some w <= 0
        tris = rng.integers(0, V, size=(T, 3)).astype(np.int32)
        ids, bary, z = oracle.forward(clip, tris, W, H)
        r_ids, r_bary, r_z = oracle.reference_forward(clip, tris, W, H)
        assert bits_equal(ids, r_ids) and bits_equal(bary, r_bary) and bits_equal(z, r_z)
        g = rng.normal(size=(H, W, 3)).astype(np.float32)
        assert bits_equal(oracle.backward(g, clip, tris, ids, bary),
                          oracle.reference_backward(g, clip, tris, r_ids, r_bary))


def test_threaded_equals_serial():
    job = synthetic.sphere_job(4, 96, 64, 10)
    a = oracle.forward(job["clip"].numpy(), job["triangles"].numpy(), 96, 64, threads=1)
    b = oracle.forward(job["clip"].numpy(), job["triangles"].numpy(), 96, 64, threads=4)
    assert all(bits_equal(x, y) for x, y in zip(a, b))


# ---- shading oracle (torch CPU restatement of rasterize() / render()) ---------------------------

def _t(a, grad=False):
    t = torch.from_numpy(np.array(a))
    return t.requires_grad_(True) if grad else t


def test_shading_oracle_rasterize_unlit_cube():
    g = golden_npz("rasterize_unlit_cube_64x48.npz")
    v, a = _t(g["vertices"], True), _t(g["attributes"], True)
    out = shading.rasterize(v, a, _t(g["triangles"]), _t(g["projection"]), 64, 48, _t(g["background"]))
    np.testing.assert_allclose(out.detach().numpy(), g["out"], atol=1e-6, rtol=0)
    torch.mean(torch.abs(out - _t(g["target"]))).backward()
    np.testing.assert_allclose(v.grad.numpy(), g["dvertices"], atol=1e-6, rtol=0)
    np.testing.assert_allclose(a.grad.numpy(), g["dattributes"], atol=1e-7, rtol=0)


@pytest.mark.parametrize("name", ["render_gray_cube_64x48.npz", "render_lit_cube_64x48.npz",
                                  "render_specular_cube_64x48.npz",
                                  "render_specular_scalar_cube_64x48.npz",
                                  "render_sphere5k_128.npz"])
def test_shading_oracle_render(name):
    g = golden_npz(name)
    h, w = g["image"].shape[1:3]
    leaves = {k: _t(g[k], True) for k in ("vertices", "normals", "diffuse", "light_positions",
                                         "light_intensities")}
    spec = _t(g["specular"], True) if "specular" in g.files else None
    amb = _t(g["ambient"], True) if "ambient" in g.files else None
    shine = _t(g["shininess"]) if "shininess" in g.files else None
    img = shading.render(leaves["vertices"], _t(g["triangles"]), leaves["normals"], leaves["diffuse"],
                         _t(g["eye"]), _t(g["center"]), _t(g["up"]), leaves["light_positions"],
                         leaves["light_intensities"], w, h, specular_colors=spec,
                         shininess_coefficients=shine, ambient_color=amb)
    np.testing.assert_allclose(img.detach().numpy(), g["image"], atol=2e-6, rtol=0)
    torch.mean(torch.abs(img - _t(g["target"]))).backward()
    for k, t in leaves.items():
        np.testing.assert_allclose(t.grad.numpy(), g["d_" + k], atol=2e-6, rtol=0, err_msg=k)
    if spec is not None:
        np.testing.assert_allclose(spec.grad.numpy(), g["d_specular"], atol=2e-6, rtol=0)
    if amb is not None:
        np.testing.assert_allclose(amb.grad.numpy(), g["d_ambient"], atol=2e-6, rtol=0)


@pytest.mark.parametrize("name", ["render_shininess_vertex_filled_64x48.npz", "render_shininess_vertex_64x48.npz",
                                  "render_shininess_image_64x48.npz"])
def test_shading_oracle_shininess_gradient(name):
    """Row F1: a shininess that requires grad (per vertex / per image).  With a background pixel the
    reference's per-vertex case returns NaN for some gradients; the oracle reproduces that."""
    g = golden_npz(name)
    keys = ("vertices", "normals", "diffuse", "specular", "light_positions", "light_intensities", "ambient",
            "shininess")
    leaves = {k: _t(g[k], True) for k in keys}
    img = shading.render(leaves["vertices"], _t(g["triangles"]), leaves["normals"], leaves["diffuse"],
                         _t(g["eye"]), _t(g["center"]), _t(g["up"]), leaves["light_positions"],
                         leaves["light_intensities"], 64, 48, specular_colors=leaves["specular"],
                         shininess_coefficients=leaves["shininess"], ambient_color=leaves["ambient"],
                         fov_y=float(g["fov_y"]))
    np.testing.assert_allclose(img.detach().numpy(), g["image"], atol=2e-6, rtol=0)
    (float(g["loss_weight"]) * torch.mean(torch.abs(img - _t(g["target"])))).backward()
    for k, t in leaves.items():
        np.testing.assert_allclose(t.grad.numpy(), g["d_" + k], atol=1e-5, rtol=0, err_msg=k)
    assert np.abs(np.nan_to_num(g["d_shininess"])).max() > 1e-4


def test_shading_oracle_nine_lights_with_specular():
    """Round 4: nine lights, diffuse AND specular, ambient, a scalar shininess per image, every input
    differentiated (the reference takes any light count, render.py:304-372; the fused HIP kernels take
    them in groups of four -- nine crosses two group boundaries)."""
    g = golden_npz("render_nine_lights_64x48.npz")
    keys = ("vertices", "normals", "diffuse", "specular", "light_positions", "light_intensities", "ambient",
            "shininess")
    leaves = {k: _t(g[k], True) for k in keys}
    img = shading.render(leaves["vertices"], _t(g["triangles"]), leaves["normals"], leaves["diffuse"],
                         _t(g["eye"]), _t(g["center"]), _t(g["up"]), leaves["light_positions"],
                         leaves["light_intensities"], 64, 48, specular_colors=leaves["specular"],
                         shininess_coefficients=leaves["shininess"], ambient_color=leaves["ambient"])
    assert g["light_positions"].shape[1] == 9
    np.testing.assert_allclose(img.detach().numpy(), g["image"], atol=2e-6, rtol=0)
    (float(g["loss_weight"]) * torch.mean(torch.abs(img - _t(g["target"])))).backward()
    for k, t in leaves.items():
        assert np.abs(g["d_" + k]).max() > 1e-5, k
        np.testing.assert_allclose(t.grad.numpy(), g["d_" + k], atol=1e-5, rtol=0, err_msg=k)


def test_shading_oracle_rasterize_seventeen_attributes():
    """Round 4: rasterize() on a random triangle soup with 17 attributes and a per-attribute background
    (rasterize.py:27-152), gradients to vertices, attributes and background.  The soup is rasterized from the STORED
    clip-space vertices the golden was made from: the host's BLAS picks its matmul kernel by CPU model, and a
    last-bit difference in clip space moves sliver-triangle pixels by ~2e-6 (gradients still flow through the matmul)."""
    g = golden_npz("rasterize_soup_a17_40x30.npz")
    clip = np.load(os.path.join(GOLDEN, "rasterize_soup_a17_40x30_clip.npy"))
    np.testing.assert_allclose(shading.transform_homogeneous(_t(g["transforms"]), _t(g["vertices"])).numpy(), clip,
                               atol=1e-6, rtol=0)
    v, a, bg = _t(g["vertices"], True), _t(g["attributes"], True), _t(g["background"], True)
    out = shading.rasterize(v, a, _t(g["triangles"]), _t(g["transforms"]), 40, 30, bg, clip_bits=_t(clip))
    assert out.shape[-1] == 17
    np.testing.assert_allclose(out.detach().numpy(), g["image"], atol=1e-6, rtol=0)
    torch.mean(torch.abs(out - _t(g["target"]))).backward()
    np.testing.assert_allclose(v.grad.numpy(), g["d_vertices"], atol=1e-6, rtol=0)
    np.testing.assert_allclose(a.grad.numpy(), g["d_attributes"], atol=1e-7, rtol=0)
    np.testing.assert_allclose(bg.grad.numpy(), g["d_background"], atol=1e-6, rtol=0)
    assert np.abs(g["d_vertices"]).max() > 1e-4


# ---- SoftRas oracle (torch CPU restatement of src/soft_mesh_renderer) -----------------------------

def test_soft_oracle_single_triangle_known_answers():
    """The reference's own 10x10 known-answer matrices (test_rasterize.py:128-215)."""
    from oracle import soft
    g = golden_npz("soft_single_triangle_10x10.npz")
    for tag in ("a", "b"):
        sig, gam, blur = g["params_" + tag]
        img = soft.rasterize_batch(_t(g["clip"]), _t(g["triangles"]), _t(g["world"]), _t(g["normals"]),
                                   _t(g["diffuse"]), _t(g["light_positions"]), _t(g["light_intensities"]),
                                   10, 10, float(sig), float(gam), float(blur))
        np.testing.assert_allclose(img.numpy(), g["image_" + tag], atol=1e-6, rtol=0)
    # case a is the hard-edged picture of the reference's docstring
    red = g["image_a"][..., 0]
    assert red[0, 9] == 1.0 and red[9, 0] == 1.0 and red[0, 0] == 0.0
    np.testing.assert_allclose(np.diag(np.fliplr(g["image_a"][..., 3])), 0.5, atol=1e-6)


def test_soft_oracle_float32_is_unchanged_by_following_the_dtype():
    """oracle/soft.py follows the dtype of its inputs (the float64 truth of tests/soft_truth.py) and reports its
    decisions through trace=.  Its float32 evaluation of the single-triangle scene reproduced the stored images
    bit for bit before that change, and must still: the stored values, not a second copy of the code, are the
    'before'.  A float64 call answers in float64, within float32 rounding of the same picture, and a trace
    changes nothing that is computed."""
    from oracle import soft
    g = golden_npz("soft_single_triangle_10x10.npz")
    args = [_t(g[k]) for k in ("clip", "triangles", "world", "normals", "diffuse", "light_positions", "light_intensities")]
    for tag in ("a", "b"):
        sig, gam, blur = [float(v) for v in g["params_" + tag]]
        img = soft.rasterize_batch(*args, 10, 10, sig, gam, blur)
        assert img.dtype == torch.float32 and torch.equal(img, _t(g["image_" + tag])), tag
        trace = {}
        assert torch.equal(soft.rasterize_batch(*args, 10, 10, sig, gam, blur, trace=trace), img)
        for key, shape in (("cand", (100, 1)), ("inside", (100, 1)), ("keep", (100, 1)), ("edge", (100, 1)),
                           ("bc", (100, 1, 3)), ("edge_dist", (100, 1, 3)), ("sq_dist", (100, 1)), ("t_raw", (100, 1)),
                           ("t_raw_edges", (100, 1, 3)), ("z", (100, 1)), ("ndl_raw", (100, 1, 1)), ("lo", (1, 2)),
                           ("hi", (1, 2)), ("area", (1,)), ("valid", (1,)), ("p2", (100, 2))):
            assert tuple(trace[key].shape) == shape and not trace[key].requires_grad, key
        wide = [a.double() if a.is_floating_point() else a for a in args]
        img64 = soft.rasterize_batch(*wide, 10, 10, sig, gam, blur)
        assert img64.dtype == torch.float64
        np.testing.assert_allclose(img64.numpy(), g["image_" + tag], atol=1e-6, rtol=0)


def test_soft_oracle_point_to_segment_nearest():
    """The vectors the reference's own test holds for point_to_segment_nearest (test_rasterize.py:9-44:
    the first three cases, with the answers written there) and 256 more through the reference function
    (rasterize.py:169-176): nearest point, parameter t and squared distance of oracle/soft.py's
    vectorised restatement."""
    from oracle import soft
    g = golden_npz("soft_point_to_segment_nearest.npz")
    p, a, b = _t(g["p"]), _t(g["a"]), _t(g["b"])
    n = p.shape[0]
    # one (pixel, triangle) pair per case: p [n,1,2] against a / b [1,n,2], the diagonal is the case itself
    d2, t = soft._nearest_on_segment(p.reshape(n, 1, 2), a.reshape(1, n, 2), b.reshape(1, n, 2))
    d2, t = torch.diagonal(d2).numpy(), torch.diagonal(t).numpy()
    np.testing.assert_allclose(t[:3], g["held_t"], atol=1e-6, rtol=0)   # the reference test's own answers (its assert_close)
    x = g["a"] + t[:, None] * (g["b"] - g["a"])
    np.testing.assert_allclose(x[:3], g["held_nearest"], atol=1e-6, rtol=0)
    np.testing.assert_allclose(t, g["t"], atol=1e-6, rtol=0)
    np.testing.assert_allclose(x, g["nearest"], atol=1e-6, rtol=0)
    want_d2 = ((g["nearest"] - g["p"]) ** 2).sum(-1)
    np.testing.assert_allclose(d2, want_d2, atol=1e-6, rtol=1e-5)
    assert (g["t"] == 0).sum() > 20 and (g["t"] == 1).sum() > 20 and ((g["t"] > 0) & (g["t"] < 1)).sum() > 20


@pytest.mark.parametrize("name", ["soft_sphere_k6_32.npz", "soft_sphere_k10_32.npz"])
def test_soft_oracle_sphere(name):
    from oracle import soft
    g = golden_npz(name)
    sig, gam = g["params"]
    leaves = {k: _t(g[k], True) for k in ("vertices", "diffuse", "light_positions")}
    b = g["vertices"].shape[0]
    img = soft.render(leaves["vertices"], _t(g["triangles"]), leaves["diffuse"], _t(g["eye"]),
                      torch.zeros(b, 3), torch.tensor(b * [[0.0, 1.0, 0.0]]), leaves["light_positions"],
                      _t(g["light_intensities"]), 32, 32, sigma_val=float(sig), gamma_val=float(gam))
    np.testing.assert_allclose(img.detach().numpy()[..., 3], g["image"][..., 3], atol=1e-6, rtol=0)
    np.testing.assert_allclose(img.detach().numpy(), g["image"], atol=5e-5, rtol=0)
    torch.mean(torch.abs(img - _t(g["target"]))).backward()
    for k, t in leaves.items():
        np.testing.assert_allclose(t.grad.numpy(), g["d_" + k], atol=5e-5, rtol=0, err_msg=k)


@pytest.mark.parametrize("name,w,h", [("clip_external_triangle.npz", 160, 120),
                                      ("clip_camera_inside_cube.npz", 160, 120)])
def test_oracle_matches_reference_on_clipping_scenes(name, w, h):
    """Vertices behind the eye: the full-screen-bbox path of rasterize_triangles.cpp:356-360."""
    g = golden_npz(name)
    ids, bary, z = oracle.forward(g["clip"], g["triangles"], w, h)
    assert bits_equal(ids, g["ids"]) and bits_equal(bary, g["bary"]) and bits_equal(z, g["z"])
    seed = 4 if "external" in name else 6
    d = oracle.backward(seeded_dbary((h, w, 3), seed=seed).numpy(), g["clip"], g["triangles"], ids, bary)
    assert bits_equal(d, g["dclip"])


@pytest.mark.parametrize("name", ["Barycentrics_Cube.png", "Simple_Tetrahedron.png"])
def test_oracle_reproduces_the_references_unused_barycentric_fixtures(name):
    """test_data/Barycentrics_Cube.png and Simple_Tetrahedron.png (held by the reference, loaded by none of its tests)
    under the reference's own comparison (test_utils.py:105-160: at most 0.1 % of the pixels off by more than 0.01)."""
    from conftest import barycentric_png_scenes, png_outlier_fraction
    clip, tris = barycentric_png_scenes()[name]
    ids, bary, z = oracle.forward(clip, tris, 640, 480)
    assert png_outlier_fraction(name, bary) <= 0.001
    if oracle.have_reference_kernel():
        ref = oracle.reference_forward(clip, tris, 640, 480)
        assert bits_equal(ids, ref[0]) and bits_equal(bary, ref[1]) and bits_equal(z, ref[2])


def test_python_kernel_capture_documents_the_z_convention():
    """SURVEY row A11 (documentation, not a parity target): the reference's DEFAULT kernel,
    rasterize_triangles_python.py:33-133, draws the same pixels as the C++ kernel this package
    reproduces, but its z output is the screen-space-interpolated viewport depth in [0, 1]
    (:122-125), not the perspective-correct NDC depth in [-1, 1] of rasterize_triangles.cpp:395-397.
    Both values of USE_CPP_RASTERIZER select the C++ semantics here."""
    py, cpp = golden_npz("python_kernel_cube64.npz"), golden_npz("raster_cube64.npz")
    covered_py, covered_cpp = py["bary"].sum(-1) > 0.5, cpp["bary"].sum(-1) > 0.5
    assert np.array_equal(covered_py, covered_cpp)                  # identical coverage
    assert int((py["ids"] != cpp["ids"]).sum()) <= 1                # one id differs on an edge
    same = covered_cpp & (py["ids"] == cpp["ids"])
    np.testing.assert_allclose(py["bary"][same], cpp["bary"][same], atol=2e-4)
    zc, zp = cpp["z"][same], py["z"][same]
    assert np.abs(zp - zc).max() > 1e-4                             # NOT the same quantity:
    np.testing.assert_allclose(zp, 0.5 * zc + 0.5, atol=1e-5)       # viewport depth (z_ndc + 1) / 2 in [0, 1]


def test_truth64_pullback_is_the_references_backward_in_float64():
    """oracle/truth64.py (what the specialised backward kernels are held against on sliver soups) evaluates the
    formulas of rasterize_triangles.cpp:131-273 in binary64: on the reference's own goldens its result is the
    reference's binary32 result up to the latter's rounding -- well inside the noise scale it reports."""
    from oracle import truth64
    g = golden_npz("raster_cube64.npz")
    d, noise = truth64.raster_pullback(g["clip"][None], g["triangles"], g["ids"][None], g["bary"][None],
                                       g["dbary"][None].astype(np.float64))
    assert np.abs(d[0] - g["dclip"]).max() < 2e-9 and np.all(d[0][:, 2] == 0.0)
    truth64.assert_within_rounding(g["dclip"][None], d, noise, "cube64", k_rounding=4.0)
    t = golden_npz("raster_triangles_160x120.npz")
    dbary = seeded_dbary((120, 160, 3), seed=1).numpy().astype(np.float64)
    for case in TRIANGLE_CASES:
        d, noise = truth64.raster_pullback(t[case + ".clip"][None], t[case + ".triangles"], t[case + ".ids"][None],
                                           t[case + ".bary"][None], dbary[None])
        truth64.assert_within_rounding(t[case + ".dclip"][None], d, noise, case, k_rounding=4.0)
        np.testing.assert_allclose(d[0], t[case + ".dclip"], atol=1e-5 * max(np.abs(t[case + ".dclip"]).max(), 1e-30), rtol=0)


@pytest.mark.parametrize("name", ["render_gray_cube_64x48.npz", "render_lit_cube_64x48.npz",
                                  "render_specular_scalar_cube_64x48.npz", "render_nine_lights_64x48.npz"])
def test_truth64_phong_is_the_references_autograd_in_float64(name):
    """truth64.phong + raster_pullback on the G-buffer of a reference golden scene reproduce the reference's image
    and every gradient it stored (render.py:201-215,287-386 through its float32 autograd) to 1e-5 of each
    gradient's largest element."""
    from truth_helpers import golden_scene_truth, golden_transforms
    g = golden_npz(name)
    B, H, W = g["image"].shape[:3]
    xf = golden_transforms(g)
    clip = shading.transform_homogeneous(xf, _t(g["vertices"])).numpy()
    ids, bary = np.zeros((B, H, W), np.int32), np.zeros((B, H, W, 3), np.float32)
    for b in range(B):
        ids[b], bary[b], _ = oracle.forward(clip[b], g["triangles"], W, H)
    out = golden_scene_truth(g, ids, bary, clip, xf.numpy())
    np.testing.assert_allclose(out["image"], g["image"], atol=2e-6, rtol=0)
    for key in ("vertices", "normals", "diffuse", "light_positions", "light_intensities", "ambient", "specular"):
        if "d_" + key in g.files:
            want = g["d_" + key]
            np.testing.assert_allclose(out["d_" + key], want, atol=1e-5 * np.abs(want).max(), rtol=0, err_msg=key)
    truth64.assert_within_rounding(g["d_vertices"], out["d_vertices"], out["noise_vertices"], name, k_rounding=4.0)
