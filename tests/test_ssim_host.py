"""SSIM loss, the part that needs no GPU: the float64 restatement (tests/ssim_reference.py) against an independent
spelling and against finite differences, the argument checks of losses.ssim / photometric_loss, and the C ABI's."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_mesh_renderer_amd import _native
from pytorch_mesh_renderer_amd.mesh_renderer import losses
from ssim_reference import noise_pair, noisy_copy, ssim_reference, window

WINDOWS = [(11, 1.5), (7, 1.0), (3, 0.8)]


def direct_map(x, y, window_size, sigma, padding, c1, c2):
    """The definition as a double loop over the window, pixel by pixel: no separable passes, no padded arrays."""
    B, H, W, C = x.shape
    g = window(window_size, sigma)
    r = window_size // 2
    off = 0 if padding == "same" else r
    Hm, Wm = (H, W) if padding == "same" else (H - window_size + 1, W - window_size + 1)
    out = np.zeros((B, Hm, Wm, C))
    for b in range(B):
        for c in range(C):
            for py in range(Hm):
                for px in range(Wm):
                    mx = my = exx = eyy = exy = 0.0
                    for i in range(window_size):
                        for j in range(window_size):
                            qy, qx = py + off - r + i, px + off - r + j
                            if 0 <= qy < H and 0 <= qx < W:
                                w, xv, yv = g[i] * g[j], float(x[b, qy, qx, c]), float(y[b, qy, qx, c])
                                mx += w * xv
                                my += w * yv
                                exx += w * xv * xv
                                eyy += w * yv * yv
                                exy += w * xv * yv
                    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
                    out[b, py, px, c] = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    return out


@pytest.mark.parametrize("padding", ["same", "valid"])
def test_restatement_agrees_with_a_direct_double_loop(padding):
    x, y = noisy_copy((1, 9, 10, 2), seed=3, amplitude=0.2)
    for window_size, sigma in WINDOWS + [(9, 2.0)]:
        if padding == "valid" and window_size > 9:
            continue                      # no window of 11 lies inside a 9 x 10 image
        ref = ssim_reference(x, y, window_size, sigma, padding)
        want = direct_map(x, y, window_size, sigma, padding, 0.01 ** 2, 0.03 ** 2)
        assert ref["map"].shape == want.shape
        assert np.abs(ref["map"] - want).max() < 1e-12
        assert abs(ref["value"] - want.mean()) < 1e-12


@pytest.mark.parametrize("padding", ["same", "valid"])
def test_restatement_gradients_agree_with_central_differences(padding):
    x, y = noise_pair((1, 9, 10, 2), seed=5)
    x, y = x.astype(np.float64), y.astype(np.float64)
    upstream, h = 1.7, 1e-5
    for window_size, sigma in WINDOWS:
        if padding == "valid" and window_size > 9:
            continue
        ref = ssim_reference(x, y, window_size, sigma, padding, upstream=upstream)
        value = lambda a, b: upstream * ssim_reference(a, b, window_size, sigma, padding)["value"]
        for name, which in (("dimage", 0), ("dtarget", 1)):
            fd = np.zeros_like(x)
            for idx in np.ndindex(*x.shape):
                step = np.zeros_like(x)
                step[idx] = h
                plus = value(x + step, y) if which == 0 else value(x, y + step)
                minus = value(x - step, y) if which == 0 else value(x, y - step)
                fd[idx] = (plus - minus) / (2 * h)
            scale = np.abs(fd).max()
            assert scale > 0
            assert np.abs(ref[name] - fd).max() <= 1e-7 * scale, (name, window_size, np.abs(ref[name] - fd).max() / scale)


def test_argument_checks_raise_before_anything_reaches_the_library():
    f = lambda *shape: torch.zeros(*shape)
    img = f(2, 12, 13, 4)
    cases = [
        ((img, f(2, 12, 13, 3)), {}, ValueError, "same shape"),
        ((f(12, 13, 4), f(12, 13, 4)), {}, ValueError, r"\[B, H, W, C\]"),
        ((img.double(), img.double()), {}, RuntimeError, "float32"),
        ((img, img.half()), {}, RuntimeError, "float32"),
        ((f(2, 12, 13, 5), f(2, 12, 13, 5)), {}, ValueError, "channels"),
        ((f(0, 12, 13, 4), f(0, 12, 13, 4)), {}, ValueError, "at least one image"),
        ((img, img), {"window_size": 4}, ValueError, "window_size"),
        ((img, img), {"window_size": 13}, ValueError, "window_size"),
        ((img, img), {"window_size": 1}, ValueError, "window_size"),
        ((img, img), {"window_size": 7.0}, ValueError, "window_size"),
        ((img, img), {"sigma": 0.0}, ValueError, "sigma"),
        ((img, img), {"sigma": -1.0}, ValueError, "sigma"),
        ((img, img), {"sigma": float("nan")}, ValueError, "sigma"),
        ((img, img), {"padding": "reflect"}, ValueError, "padding"),
        ((f(1, 10, 30, 4), f(1, 10, 30, 4)), {"padding": "valid"}, ValueError, "valid"),
        ((f(1, 30, 6, 4), f(1, 30, 6, 4)), {"padding": "valid", "window_size": 7}, ValueError, "valid"),
        ((img, img), {"k2": 0.0}, ValueError, "k2"),          # C2 = 0: 0 / 0 wherever both images are flat
        ((img, img), {"k1": 0.0}, ValueError, "k1"),
        ((img, img), {"k1": -0.01}, ValueError, "k1"),
        ((img, img), {"data_range": 0.0}, ValueError, "data_range"),
        ((img, img), {"data_range": float("inf")}, ValueError, "data_range"),
        ((img, img), {"k2": float("nan")}, ValueError, "k2"),
        ((img, img), {"k1": 1e-30}, ValueError, "float32"),   # squares to zero
        ((img, img), {"window": 7}, TypeError, "window"),     # an unknown keyword
    ]
    for args, kwargs, exc, word in cases:
        with pytest.raises(exc, match=word):
            losses.ssim(*args, **kwargs)
        with pytest.raises(exc, match=word):
            losses.photometric_loss(*args, **kwargs)
    # photometric_loss checks the SSIM arguments at every weight, also where the SSIM part is not computed
    for weight in (0.0, 0, 1.0):
        for kwargs, exc, word in (({"k2": 0.0}, ValueError, "k2"), ({"window": 7}, TypeError, "window"),
                                  ({"padding": "reflect"}, ValueError, "padding")):
            with pytest.raises(exc, match=word):
                losses.photometric_loss(img, img, ssim_weight=weight, **kwargs)
    with pytest.raises(ValueError, match="c1 and c2"):
        _native.ssim_forward(img, img, c2=0.0)
    for weight in (-0.1, 1.5, float("nan"), "0.2", None):
        with pytest.raises(ValueError, match="ssim_weight"):
            losses.photometric_loss(img, img, ssim_weight=weight)
    # well-formed CPU tensors get past the checks and are refused for the device only
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.ssim(img, img)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.ssim(f(1, 5, 70, 3), f(1, 5, 70, 3))      # shorter than the window: legal under "same"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.ssim(img.permute(0, 2, 1, 3), img.permute(0, 2, 1, 3), window_size=3, sigma=0.8, padding="valid")
    # the native wrappers repeat the checks: nothing reaches the library unchecked
    with pytest.raises(RuntimeError, match="float32"):
        _native.ssim_forward(img.double(), img.double())
    with pytest.raises(ValueError, match="grads"):
        _native.ssim_forward(img, img, grads=4)
    with pytest.raises(ValueError, match="saved"):
        _native.ssim_backward(img, img, f(7), f(1), grads=1)
    with pytest.raises(ValueError, match="saved nothing"):
        _native.ssim_backward(img, img, f(3 * img.numel()), f(1), grads=1, want_image=False, want_target=True)


def test_abi_rejects_bad_arguments_before_touching_a_device():
    L = _native.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)   # never dereferenced: every call below fails its checks
    SAME, VALID = _native.SSIM_SAME, _native.SSIM_VALID
    # size queries: 0 for a bad argument, the tile / plane counts otherwise
    assert L.mr_ssim_partials(2, 37, 45, 11, SAME) == 2 * 3 * 2            # 32 x 16 tiles of a 45 x 37 map
    assert L.mr_ssim_partials(2, 37, 45, 11, VALID) == 2 * 2 * 2           # ... of a 35 x 27 map
    assert L.mr_ssim_partials(32, 1024, 1024, 11, SAME) == 32 * 64 * 32
    assert L.mr_ssim_saved_floats(2, 37, 45, 4, 11, SAME, 1) == 3 * 2 * 37 * 45 * 4
    assert L.mr_ssim_saved_floats(2, 37, 45, 3, 11, SAME, 2) == 3 * 2 * 37 * 45 * 3
    assert L.mr_ssim_saved_floats(2, 37, 45, 4, 11, VALID, 3) == 4 * 2 * 27 * 35 * 4
    assert L.mr_ssim_saved_floats(32, 1024, 1024, 4, 11, SAME, 1) == 3 * 32 * 1024 * 1024 * 4   # > 2^32 bytes
    for bad in ((0, 8, 8, 11, SAME), (-1, 8, 8, 11, SAME), (70000, 8, 8, 11, SAME), (1, 0, 8, 11, SAME),
                (1, 8, 70000, 11, SAME), (1, 8, 8, 4, SAME), (1, 8, 8, 13, SAME), (1, 8, 8, 1, SAME), (1, 8, 8, 11, 2),
                (1, 8, 30, 11, VALID), (1, 30, 8, 11, VALID)):
        assert L.mr_ssim_partials(*bad) == 0, bad
        B, H, W, window, padding = bad
        assert L.mr_ssim_saved_floats(B, H, W, 4, window, padding, 1) == 0, bad
    assert L.mr_ssim_saved_floats(1, 8, 8, 0, 11, SAME, 1) == 0
    assert L.mr_ssim_saved_floats(1, 8, 8, 5, 11, SAME, 1) == 0
    assert L.mr_ssim_saved_floats(1, 8, 8, 4, 11, SAME, 0) == 0
    assert L.mr_ssim_saved_floats(1, 8, 8, 4, 11, SAME, 4) == 0

    def forward(B=1, H=8, W=8, C=4, window=11, sigma=1.5, c1=1e-4, c2=9e-4, padding=SAME, grads=0, image=one,
                target=one, mean=one, ssim_map=null, saved=null, partials=one):
        return L.mr_ssim_forward(image, target, B, H, W, C, window, sigma, c1, c2, padding, grads, mean, ssim_map, saved,
                                 partials, null)

    def backward(B=1, H=8, W=8, C=4, window=11, sigma=1.5, padding=SAME, grads=1, image=one, target=one, saved=one,
                 upstream=one, da=one, db=null):
        return L.mr_ssim_backward(image, target, saved, upstream, B, H, W, C, window, sigma, padding, grads, da, db, null)

    E = _native.MR_EINVAL
    for kwargs in ({"B": 0}, {"B": 65536}, {"H": 0}, {"W": -3}, {"C": 0}, {"C": 5}, {"window": 4}, {"window": 13},
                   {"sigma": 0.0}, {"sigma": float("nan")}, {"sigma": float("inf")}, {"c1": -1.0}, {"c1": 0.0},
                   {"c2": 0.0}, {"c2": float("nan")},
                   {"padding": 2}, {"padding": VALID}, {"grads": 4}, {"grads": -1}, {"image": null}, {"target": null},
                   {"mean": null}, {"partials": null}, {"grads": 1},                      # grads without a saved block
                   {"image": ctypes.c_void_p(20)}, {"ssim_map": ctypes.c_void_p(20)}):   # C = 4: 16-byte alignment
        assert forward(**kwargs) == E, kwargs
    for kwargs in ({"B": 0}, {"H": 70000}, {"C": 5}, {"window": 6}, {"sigma": -1.0}, {"padding": VALID}, {"grads": 0},
                   {"grads": 4}, {"image": null}, {"saved": null}, {"upstream": null},
                   {"grads": 2},                                    # d image from planes saved for the target only
                   {"grads": 1, "db": one}, {"da": ctypes.c_void_p(24)}):
        assert backward(**kwargs) == E, kwargs


def test_new_symbols_are_exported_and_the_abi_version_stays():
    L = _native.lib()
    for name in ("mr_ssim_partials", "mr_ssim_saved_floats", "mr_ssim_forward", "mr_ssim_backward"):
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert L.mr_version() == 356 == _native.ABI_VERSION
    assert callable(losses.ssim) and callable(losses.photometric_loss)
