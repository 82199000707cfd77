"""GPU parity of the SPECIALISED backward kernels: each one directly on the reference's stored gradients, and on
random soups against the float64 truth (oracle/truth64.py) within a stated rounding bound.

The general kernels (k_accumulate_rows: every gradient wanted) are what the golden tests of test_render_gpu.py run,
because those make every leaf require grad.  render() picks other pixel passes when fewer gradients are wanted --
ShadeFoldLaneFn (vertices only: the benchmark's kernel), ShadeDiffLaneFn (vertices + normals and / or diffuse),
SpecFoldLaneFn (specular, vertices only) -- and rasterize() picks AttrFoldLaneFn on its own G-buffer.  Here the
reference's goldens (/root/reference/src/mesh_renderer/render.py:304-372 through its autograd) are re-run with
exactly those leaves requiring grad, through both loss spellings, and the kernel that ran is checked by name.
"""
import numpy as np
import pytest
import torch

import backward_fuzz
from conftest import golden_npz
from oracle import truth64
from pytorch_mesh_renderer_amd import _native, mesh_renderer
from truth_helpers import golden_scene_truth, golden_transforms

pytestmark = pytest.mark.gpu
ATOL = 1e-4   # north_star: shaded RGBA and gradients within 1e-4 abs

DIFFUSE = ["render_gray_cube_64x48.npz", "render_lit_cube_64x48.npz", "render_sphere5k_128.npz",
           "render_six_lights_64x48.npz"]
SPECULAR = ["render_specular_cube_64x48.npz", "render_specular_scalar_cube_64x48.npz",
            "render_shininess_image_64x48.npz", "render_shininess_vertex_64x48.npz",
            "render_shininess_vertex_filled_64x48.npz", "render_nine_lights_64x48.npz"]


def _render(g, device, wanted, spelling):
    """The golden scene with only the leaves in `wanted` requiring grad -> (image, {leaf: grad}, kernel name)."""
    h, w = g["image"].shape[1:3]
    dev = lambda k: torch.tensor(g[k], device=device)
    leaves = {k: dev(k).requires_grad_(k in wanted) for k in ("vertices", "normals", "diffuse")}
    lights = {k: dev(k).requires_grad_(k in wanted) for k in ("light_positions", "light_intensities")}
    spec = dev("specular") if "specular" in g.files else None
    shine = dev("shininess") if "shininess" in g.files else None
    amb = dev("ambient") if "ambient" in g.files else None
    kw = {"fov_y": float(g["fov_y"])} if "fov_y" in g.files else {}
    img = mesh_renderer.render(leaves["vertices"], dev("triangles"), leaves["normals"], leaves["diffuse"], dev("eye"),
                               dev("center"), dev("up"), lights["light_positions"], lights["light_intensities"], w, h,
                               specular_colors=spec, shininess_coefficients=shine, ambient_color=amb, **kw)
    weight = float(g["loss_weight"]) if "loss_weight" in g.files else 1.0
    if spelling == "mean_abs":     # the reference's own spelling, mesh_renderer_test.py:250
        loss = torch.mean(torch.abs(img - dev("target")))
    elif spelling == "generic_op":   # the loss as an op of its own: the renderer's node gets the dense gradient image
        mesh_renderer.losses.USE_FUSED_RENDER_LOSS = False
        try:
            loss = mesh_renderer.losses.l1_loss(img, dev("target"))
        finally:
            mesh_renderer.losses.USE_FUSED_RENDER_LOSS = True
    else:
        loss = mesh_renderer.losses.l1_loss(img, dev("target"))
    (loss * weight).backward()
    torch.cuda.synchronize()
    grads = {k: t.grad for k, t in list(leaves.items()) + list(lights.items()) if t.requires_grad}
    return img, grads, _native.debug_last_accumulate_kernel()


def _compare(g, grads, what):
    for k, got in grads.items():
        assert got is not None, k
        want = g["d_" + k]
        ok = np.isfinite(want)   # per-vertex shininess + background: some of the reference's own entries are NaN
        got = got.cpu().numpy()
        assert np.isfinite(got).all(), (what, k)
        if not ok.any():   # (the reference's whole gradient is NaN there: only finiteness to check)
            continue
        np.testing.assert_allclose(got[ok], want[ok], atol=ATOL, rtol=0, err_msg="%s: d %s" % (what, k))
        # 1e-4 abs is loose against gradients of 1e-3: also within 2e-3 of the gradient's largest element
        assert np.abs(got[ok] - want[ok]).max() <= 2e-3 * np.abs(want[ok]).max() + 1e-7, (what, k)


@pytest.mark.parametrize("spelling", ["mean_abs", "l1_loss"])
@pytest.mark.parametrize("wanted,kernel", [(("vertices",), "ShadeFoldLaneFn"), (("vertices", "normals"), "ShadeDiffLaneFn"),
                                           (("vertices", "diffuse"), None), (("vertices", "normals", "diffuse"), "ShadeDiffLaneFn")])
@pytest.mark.parametrize("name", DIFFUSE)
def test_diffuse_goldens_through_the_specialised_backward_kernels(device, name, wanted, kernel, spelling):
    g = golden_npz(name)
    img, grads, ran = _render(g, device, wanted, spelling)
    np.testing.assert_allclose(img.detach().cpu().numpy(), g["image"], atol=ATOL, rtol=0)
    if kernel is not None:
        assert ran.startswith(kernel), "%s with %s requiring grad ran %s" % (name, wanted, ran)
    _compare(g, grads, "%s %s %s (%s)" % (name, wanted, spelling, ran))


@pytest.mark.parametrize("spelling", ["mean_abs", "l1_loss"])
@pytest.mark.parametrize("wanted", [("vertices", "light_positions", "light_intensities"),
                                    ("vertices", "normals", "diffuse", "light_positions", "light_intensities")])
@pytest.mark.parametrize("name", ["render_gray_cube_64x48.npz", "render_lit_cube_64x48.npz", "render_sphere5k_128.npz"])
def test_diffuse_goldens_with_light_gradients_through_the_lane_kernel(device, name, wanted, spelling):
    """Round 5: one or two lights WITH their gradients take the difference-basis lane kernel too (ShadeDiffLaneFn<...,
    LG>: the light sums ride along per lane), folded to world space when the cameras are not differentiated."""
    g = golden_npz(name)
    img, grads, ran = _render(g, device, wanted, spelling)
    assert ran.startswith("ShadeDiffLaneFn") and ran.rstrip(">").endswith("true, true"), ran   # <L, SIGNS, GROUPS, FOLD, LG>
    _compare(g, grads, "%s %s %s (%s)" % (name, wanted, spelling, ran))


@pytest.mark.parametrize("spelling", ["mean_abs", "l1_loss", "generic_op"])
@pytest.mark.parametrize("name", SPECULAR)
def test_specular_goldens_through_the_vertex_only_lane_kernel(device, name, spelling):
    """render() with a specular term differentiated to the vertices alone: SpecFoldLaneFn with the clip-space
    pull-back folded in (one or two lights: SpecCoupledLaneFn, the across-pixels coupling in the same pass), against the
    reference's stored d_vertices."""
    g = golden_npz(name)
    img, grads, ran = _render(g, device, ("vertices",), spelling)
    np.testing.assert_allclose(img.detach().cpu().numpy(), g["image"], atol=ATOL, rtol=0)
    n_lights = g["light_positions"].shape[1]
    if n_lights <= 2:      # round 5: one pass, no separate G pass (SpecCoupledLaneFn<L, PV>)
        assert ran.startswith("SpecCoupledLaneFn<%d" % n_lights), ran
        # <L, PV, SIGNS>: the loss's sign codes go straight into the pixel pass unless the loss is an op of its own
        # (the compiler's name leaves a defaulted SIGNS = false out: "<2, true>" is <L = 2, PV = true>)
        assert (ran.count(",") == 2 and ran.endswith(", true>")) == (spelling != "generic_op"), ran
    elif n_lights <= _native.shade_fast_lights():
        assert ran.startswith("SpecFoldLaneFn") and ran.rstrip(">").endswith("true"), ran   # <L, PV, FOLD = true>
    _compare(g, grads, "%s vertices %s (%s)" % (name, spelling, ran))


@pytest.mark.parametrize("name", SPECULAR)
def test_specular_goldens_with_every_gradient_through_the_l1_entry(device, name):
    """mr_shade_specular_backward_l1 outside its one-pass case (every leaf wants a gradient: SpecGradFn, the dense image
    formed inside the call) equals the reference's stored gradients, and the generic op's to 1e-5 of their scale."""
    g = golden_npz(name)
    wanted = ("vertices", "normals", "diffuse", "light_positions", "light_intensities")
    _, grads, ran = _render(g, device, wanted, "mean_abs")
    assert ran.startswith("SpecGradFn"), ran
    _compare(g, grads, "%s all gradients, l1 entry" % name)
    _, generic, _ = _render(g, device, wanted, "generic_op")
    for k in grads:   # (the same kernels on the same dense image; their float atomics reorder the sums from run to run)
        scale = float(generic[k].abs().max())
        assert float((grads[k] - generic[k]).abs().max()) <= 1e-5 * scale + 1e-12, k


def test_specular_lane_kernel_with_its_own_clip_gradient_matches_reference_golden(device):
    """The UNFOLDED form of SpecFoldLaneFn (clip-space gradient wanted on its own: 18 sums) on the reference's scene:
    G-buffer from the device, d clip and d positions separately, recombined on the host with the reference's
    transform and compared with its d_vertices -- and with the float64 truth within the rounding bound."""
    for name in ("render_specular_scalar_cube_64x48.npz", "render_specular_cube_64x48.npz"):
        g = golden_npz(name)
        B, H, W = g["image"].shape[:3]
        xf = golden_transforms(g)
        t = lambda a: torch.tensor(np.ascontiguousarray(a), device=device)
        clip = _native.vertex_transform(t(g["vertices"]), xf.to(device))
        ids, bary, _ = _native.rasterize_forward(clip, t(g["triangles"]), W, H)
        shin = g["shininess"] if g["shininess"].ndim else np.full((B,), float(g["shininess"]), np.float32)
        args = [t(g[k]) for k in ("normals", "vertices", "diffuse", "specular", "triangles", "light_positions", "light_intensities", "ambient")]
        rgba, norms2 = _native.shade_specular_forward(ids, bary, *args, t(g["eye"]), t(shin))
        np.testing.assert_allclose(rgba.cpu().numpy(), g["image"], atol=ATOL, rtol=0)
        drgba = (torch.sign(rgba - t(g["target"])) / rgba.numel()).contiguous()
        adjacency = _native.vertex_adjacency(t(g["triangles"]), g["vertices"].shape[1])
        out = _native.shade_specular_backward(drgba, ids, bary, clip, *args, t(g["eye"]), t(shin), norms2, adjacency=adjacency,
                                              normalised_gbuffer=True, grads_wanted=_native.GRAD_POSITIONS | _native.GRAD_CLIP)
        ran = _native.debug_last_accumulate_kernel()
        assert ran.startswith("SpecFoldLaneFn") and ran.rstrip(">").endswith("false"), ran
        whole = out[2].cpu().numpy() + np.einsum("bkc,bvk->bvc", xf.numpy()[:, :, :3], out[0].cpu().numpy())
        np.testing.assert_allclose(whole, g["d_vertices"], atol=ATOL, rtol=0)
        assert np.abs(whole - g["d_vertices"]).max() <= 2e-3 * np.abs(g["d_vertices"]).max()
        truth = golden_scene_truth(g, ids.cpu().numpy(), bary.cpu().numpy(), clip.cpu().numpy(), xf.numpy())
        truth64.assert_within_rounding(out[0].cpu().numpy(), truth["d_clip"], truth["noise_clip"], name + " d clip")


def test_recorded_fuzz_failure_is_adjudicated_against_float64(device):
    """The one failure the round-4 lane-variant fuzzer recorded (seed 17, trial 43: the specular lane kernel and the rows
    kernel 3 % of the largest element apart at three vertices).  The soup is committed; each of the three kernels is held
    against the float64 truth on its own, within the rounding bound -- i.e. the disagreement is two binary32
    evaluations of an ill-conditioned sum, not a bookkeeping error of either."""
    s = golden_npz("soup_spec_sliver_seed17_trial43.npz")
    report = backward_fuzz.Report()
    backward_fuzz.specular_case(report, "seed 17 trial 43", s["positions"], s["transforms"], s["triangles"], s["normals"],
                                s["diffuse"], s["specular"], s["light_positions"], s["light_intensities"], s["ambient"],
                                s["camera"], s["shininess"], s["upstream"].copy(), int(s["W"]), int(s["H"]))
    print("excess over the rounding bound per kernel:", report.summary())
    assert not report.failures, "\n".join(report.failures)
    assert report.with_gradients == 1


def test_fuzz_harness_reports_a_changed_input_and_leaves_its_evidence(device, tmp_path, monkeypatch):
    """The harness's own plumbing (round 6): a device input that changes under the backward calls -- here a vertex
    normal, edited after the first call by a wrapper standing in for a stray write -- is reported BY NAME, the kernels
    that ran after it are beyond the bound, and the case's inputs, truth and outputs are in the .npz the message names."""
    import numpy as np
    real = _native.shade_specular_backward
    calls = []

    def stray_write(*args, **kw):
        out = real(*args, **kw)
        if not calls:
            args[4][0, :, :] += 3.0          # normals of image 0, after the rows kernel's call
        calls.append(1)
        return out
    monkeypatch.setattr(_native, "shade_specular_backward", stray_write)
    report = backward_fuzz.Report(dump_dir=str(tmp_path))
    rng = np.random.default_rng(11)
    backward_fuzz.specular_trial(rng, 0, report, small=True)
    text = "\n".join(report.failures)
    assert "DEVICE INPUT `normals` CHANGED under the backward calls" in text, text
    assert "SpecFoldLaneFn" in text and "SpecGradFn" not in text.split("DEVICE INPUT")[0], text   # rows ran before the write
    assert len(report.dumps) == 1 and report.dumps[0] in text
    with np.load(report.dumps[0]) as z:
        names = set(z.files)
        assert {"in/normals", "in_after/normals", "in/upstream", "in/ids", "truth/d_vertices"} <= names, sorted(names)
        assert any(n.startswith("out/SpecGradFn") for n in names) and any(n.startswith("out/SpecFoldLaneFn") for n in names)
        assert not np.array_equal(z["in/normals"], z["in_after/normals"])
    # ... and an input that is not what the truth was computed from is caught before any kernel runs
    report2 = backward_fuzz.Report(dump_dir=str(tmp_path))
    monkeypatch.setattr(_native, "shade_specular_backward", real)
    real_forward = _native.shade_specular_forward

    def late_edit(ids, bary, *rest, **kw):
        out = real_forward(ids, bary, *rest, **kw)
        if kw.get("norms2") is not None:      # the harness's last forward call: edit one barycentric afterwards
            bary[0, 0, 0, 0] += 0.25
        return out
    monkeypatch.setattr(_native, "shade_specular_forward", late_edit)
    backward_fuzz.specular_trial(np.random.default_rng(11), 0, report2, small=True)
    assert any("`bary` is not what the truth was computed from" in f for f in report2.failures), report2.failures


@pytest.mark.parametrize("which,trials", [("shade", 200), ("specular", 200), ("attr", 200), ("raster", 200)])
def test_backward_kernels_against_float64_on_random_soups(device, which, trials):
    """A fixed-seed slice of the stand-alone fuzzers inside the suite: every pixel-pass variant of the three backward
    entry points on random soups (slivers, one-pixel triangles, crowded and ragged images), each within
    backward_fuzz.K_ROUNDING * 2^-24 * (sum of |terms|) of the float64 truth (raster: mr_rasterize_backward's two kernels
    within the scene's own, tighter K_scene of raster_backward_scenes).  No retries: a trial beyond the bound
    fails the test and leaves its inputs, the truth and every kernel's outputs in an .npz (backward_fuzz.Evidence)."""
    fn = {"shade": backward_fuzz.shade_trial, "specular": backward_fuzz.specular_trial, "attr": backward_fuzz.attr_trial,
          "raster": backward_fuzz.raster_trial}[which]
    report = backward_fuzz.run(fn, trials, seed=505, small=True)
    print("%s: %d trials (%d with gradients); excess over the rounding bound per kernel: %s" % (
        which, report.trials, report.with_gradients, report.summary()))
    assert not report.failures, "%d failures, first: %s" % (len(report.failures), "\n".join(report.failures[:5]))
    assert report.with_gradients >= trials // 2
    expected = {"shade": ("ShadeGradFn/dense", "ShadeFoldLaneFn/dense", "ShadeFoldLaneFn/signs", "ShadeDiffLaneFn/dense", "ShadeDiffLaneFn/signs"),
                "specular": ("SpecGradFn", "SpecFoldLaneFn/lanes", "SpecFoldLaneFn/folded", "SpecCoupledLaneFn/folded"),
                "attr": ("AttrFoldLaneFn",), "raster": ("RasterLanesFn", "RasterGradFn/deterministic")}[which]
    for kernel in expected:
        assert kernel in report.worst, (kernel, sorted(report.worst))
    # raster: the deterministic kernel is left out of a trial beyond its fixed-point headroom -- of a quarter at most
    assert report.det_skipped <= trials // 4, report.det_skipped
