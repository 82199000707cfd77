"""k_aa_forward / k_aa_backward (csrc/antialias.hip) against the float64 truth on every scene of
tests/antialias_scenes.py, with the float atomics and under set_deterministic(True) (GPU).

The G-buffer is the DEVICE's (_native.rasterize_forward), edited on the host where the scene is a foreign one; the pair
mask must equal the restatement's exactly, and every element of out, dimage and dclip must satisfy

    |kernel - truth| <= K 2^-24 noise + 1e-7 max|truth|        K = 16, from the float32 restatement alone
                                                                 (tests/test_antialias_truth_host.py)

Deterministic mode adds its own quantisation to dclip's bound, from csrc/det_fixed.h: every wavefront commit is rounded
to a multiple of 2^-k, k = 41 - e for the largest per-wavefront sum g = m 2^e: n_commits 2^-42 2^e per element
(antialias_scenes.det_quantisation; 1e-13 .. 3e-7 here, below the floor everywhere).

Views 4 bytes into a buffer: bit-equal to aligned copies in out, dimage, the mask, and in deterministic mode dclip; the
float atomics commit in a free order, so their dclip is held to the bound instead.

MEASURED (MI355X; the largest |kernel - truth| / bound, float atomics, deterministic mode in brackets where it differs):

    scene           out     dimage  dclip             scene          out     dimage  dclip
    ragged_65x47    0.055   0.066   0.008 (0.009)     spike          0.023   0.033   0.018
    ragged_63x5     0.046   0.050   0.043             centre         0.039   0.046   0.011 (0.017)
    ragged_7x3      0.021   0.029   0.015             coplanar       0.059   0.051   0.008 (0.007)
    ragged_130x6    0.046   0.054   0.032             rolled_1       0.040   0.074   0.007 (0.014)
    ragged_1x9      0.051   0.042   0.069             rolled_2       0.052   0.053   0.006 (0.008)
    ragged_9x1      0.021   0.008   0.003             poisoned       0.048   0.065   0.007 (0.006)
    seams_sphere    0.046   0.077   0.016             scaled_*       0.078   0.100   0.023
    seams_soup      0.069   0.097   0.050             long_edge      0.055   0.062   0.009
    ragged_65x47 at C = 1, 2, 3, 5, 7: <= 0.075, 0.066, 0.013; seams_soup at C = 1, 2, 5: <= 0.072, 0.099, 0.055;
    seams_soup with the image times 1e3 / 1e-3: 0.097 0.097 0.047 / 0.095 0.097 0.067
    ragged_1x1, midpoint, no_triangles, no_images: exactly the inputs, dclip exactly zero
The kernels sit at a tenth of the bound at the worst: the model counts every rounding at full size, and of K = 16 the
factor 4 is headroom for an order of summation the kernel turns out not to need.

MUTATIONS of eval_pair / k_aa_backward (arithmetic and slot selection only, each built into a copy of the library and
run once; the worst |kernel - truth| / bound of the first failing scenes; older = tests/test_antialias_gpu.py):

    mutation                                     new tests that fail                                   older tests that fail
    va / vb swapped (r.va = vi[kb], ..)          31 of 40: dclip 4.8e4 (centre) .. 4.2e6 (ragged_1x9)  12 of 16
    sign of gw[2 k]'s second product flipped     30 of 40: dclip 8.8e4 (poisoned) .. 3.3e5 (centre)    12
    D = the rounded e(f) - e(g)                  2: seams_soup at C = 2 (2.12) and C = 5 (1.40)        1 (the 256 x 256 sphere,
                                                                                                       0.147 against 0.123)
    leader loop sums a lane's first slot only    25 of 40: dclip 2.1e3 (ragged_63x5) .. 5.3e4          12
    pair_weight(mod_f) = t - 0.5                 30 of 40: out, dimage 7e5 .. 1.7e6                    12
The rounded D is the closest call: its error is the cancellation of the edge function's constant term, which the noise
scale's conditioning term partly allows for; only the soup at 130 x 10 has pairs where it exceeds that.
"""
import numpy as np
import pytest
import torch

import antialias_reference as ref
import antialias_scenes as S
from pytorch_mesh_renderer_amd import _native

pytestmark = pytest.mark.gpu
K = S.K

_cache = {}


def on_device(name, device):
    """-> (scene, device tensors (ids, bary, z, clip, tris, opp), the restatement's pairs and mask), once per scene."""
    if name not in _cache:
        sc = S.scene(name)
        if name in S.RASTERIZED:
            raw = _native.rasterize_forward(torch.from_numpy(sc.clip).to(device), torch.from_numpy(sc.tris).to(device),
                                            sc.W, sc.H)
            raw = tuple(a.cpu().numpy() for a in raw)
        else:
            raw = S.blank_gbuffer(sc)
        ids, bary, z, tris, opp = S.assemble(sc, *raw)
        pairs, mask = ref.decide(ids, bary, z, sc.clip, tris, opp)
        dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (ids, bary, z, sc.clip, tris, opp))
        _cache[name] = (sc, dev, pairs, mask)
    return _cache[name]


def run(dev, image, dout, deterministic):
    """Forward (with the pair mask) and backward -> host arrays out, mask, dimage, dclip."""
    device = dev[0].device
    image, dout = torch.as_tensor(image).to(device), torch.as_tensor(dout).to(device)
    before = _native.set_deterministic(deterministic)
    try:
        out, mask = _native.antialias_forward(image, *dev, want_pair_mask=True)
        dimage, dclip = _native.antialias_backward(dout, image, *dev)
    finally:
        _native.set_deterministic(before)
    return tuple(a.cpu().numpy() for a in (out, mask, dimage, dclip))


def check(name, device, C=None, image_scale=1.0):
    """Both modes of one scene at one channel count against the truth -> {mode: (out, mask, dimage, dclip)}."""
    sc, dev, pairs, want_mask = on_device(name, device)
    image, dout = sc.inputs(C, image_scale)
    t = S.Truth(sc, pairs, image, dout)
    got = {}
    for mode in ("float", "deterministic"):
        out, mask, dimage, dclip = got[mode] = run(dev, image, dout, mode == "deterministic")
        assert np.array_equal(mask, want_mask), "%s: blended pairs differ at %d pixels" % (name, int((mask != want_mask).sum()))
        extra = t.det_extra if mode == "deterministic" else 0.0
        worst = {"out": ref.excess(out, t.out, t.n_out, K), "dimage": ref.excess(dimage, t.dimage, t.n_dimage, K),
                 "dclip": ref.excess(dclip, t.dclip, t.n_dclip, K, extra)}
        print("AAT | %-13s | C %d | image x %-5g | %-13s | pairs %4d | worst out %.3f dimage %.3f dclip %.3f of the bound"
              " | r32 %.2f %.2f %.2f" % (name, image.shape[3], image_scale, mode, len(pairs["b"]), worst["out"],
                                         worst["dimage"], worst["dclip"], t.r32["out"], t.r32["dimage"], t.r32["dclip"]))
        assert all(np.isfinite(a).all() for a in (out, dimage, dclip)), name
        assert not dclip[..., 2].any(), "%s: gradient to clip z" % name
        assert max(worst.values()) <= 1.0, "%s (%s): %s times the bound (K = %g)" % (name, mode, worst, K)
    return sc, got


@pytest.mark.parametrize("name", S.SCENES)
def test_every_scene_in_both_modes(device, name):
    check(name, device)


@pytest.mark.parametrize("C", S.CHANNELS)
def test_every_channel_count_on_the_ragged_cube(device, C):
    check(S.FULL_SWEEP, device, C)


@pytest.mark.parametrize("C", [1, 2, 5])
def test_generic_and_single_channel_paths_across_seams(device, C):
    check("seams_soup", device, C)


@pytest.mark.parametrize("image_scale", [1e3, 1e-3])
def test_bound_follows_the_image_scale(device, image_scale):
    for name in ("seams_soup", "rolled_2"):
        check(name, device, image_scale=image_scale)


@pytest.mark.parametrize("name", S.UNBLENDED)
def test_nothing_to_blend_copies_the_image_and_leaves_dclip_zero(device, name):
    sc, got = check(name, device)
    image, dout = sc.inputs()
    for mode, (out, mask, dimage, dclip) in got.items():
        assert out.tobytes() == image.tobytes() and dimage.tobytes() == dout.tobytes(), (name, mode)
        assert not mask.any() and not dclip.any() and dclip.shape == sc.clip.shape, (name, mode)


def test_scaling_clip_by_a_power_of_two_moves_no_bit_in_deterministic_mode(device):
    base_sc, base = check("scaled_1", device)
    _, base_dev, _, _ = on_device("scaled_1", device)
    for name in ("scaled_down", "scaled_up"):
        sc, got = check(name, device)
        _, dev, _, _ = on_device(name, device)
        assert all(torch.equal(a, b) for a, b in zip(dev[:3], base_dev[:3])), "the rasterizer's G-buffer moved"
        out, mask, dimage, dclip = got["deterministic"]
        b_out, b_mask, b_dimage, b_dclip = base["deterministic"]
        assert np.array_equal(mask, b_mask) and out.tobytes() == b_out.tobytes() and dimage.tobytes() == b_dimage.tobytes()
        scaled = dclip * np.float32(sc.scale)
        assert scaled.tobytes() == b_dclip.tobytes(), "%s: %d elements of dclip * lambda differ, by up to %.3e" % (
            name, int((scaled != b_dclip).sum()), float(np.abs(scaled.astype(np.float64) - b_dclip).max()))


def test_deterministic_mode_repeats_bit_for_bit_on_the_ragged_and_foreign_scenes(device):
    for name in ("ragged_65x47", "seams_soup", "rolled_2", "poisoned"):
        sc, dev, pairs, _ = on_device(name, device)
        image, dout = sc.inputs()
        a, b = run(dev, image, dout, True), run(dev, image, dout, True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), name


def test_views_four_bytes_into_a_buffer_equal_aligned_copies(device):
    """image, dout and clip as contiguous views starting 4 bytes into their storage (_native._aligned16 moves the
    ones the kernels read 16 bytes at a time)."""
    for name, C in (("ragged_65x47", 4), ("seams_soup", 3)):
        sc, dev, pairs, _ = on_device(name, device)
        image, dout = sc.inputs(C)

        def shifted(a):
            buf = torch.empty(a.size + 1, dtype=torch.float32, device=device)
            view = buf[1:].view(a.shape)
            view.copy_(torch.from_numpy(a))
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            return view

        for det in (False, True):
            want = run(dev, image, dout, det)
            before = _native.set_deterministic(det)
            try:
                im, do, clip = shifted(image), shifted(dout), shifted(sc.clip)
                args = (dev[0], dev[1], dev[2], clip, dev[4], dev[5])
                out, mask = _native.antialias_forward(im, *args, want_pair_mask=True)
                dimage, dclip = _native.antialias_backward(do, im, *args)
            finally:
                _native.set_deterministic(before)
            got = tuple(a.cpu().numpy() for a in (out, mask, dimage, dclip))
            same = [x.tobytes() == y.tobytes() for x, y in zip(got[:3], want[:3])]
            assert all(same), (name, det, same)
            if det:
                assert got[3].tobytes() == want[3].tobytes(), name
            else:                                                    # float atomics: the order of commits is free
                t = S.Truth(sc, pairs, image, dout)
                assert ref.excess(got[3], t.dclip, t.n_dclip, K) <= 1.0
