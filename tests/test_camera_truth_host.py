"""The camera families of tests/camera_reference.py are fit to judge a kernel by (no GPU needed): clear of look_at's
degeneracy cut-off by a wide margin in both precisions, every truth gradient alive, the float32 and float64
restatements agreeing on the flags, the Jacobian consistent with the weighted gradients.

MEASURED (600 cameras, seed 5; one x86 host -- r is a property of the host's float32 and moves by up to 2x between
CPUs): the float32 restatement's worst per-camera relative error r by family and tensor, and the smallest lengths

    family            matrix    d eye     d center  d up      min f_len  min s_len    (at B = 257: f_len, s_len)
    plain             5.3e-7    1.7e-6    2.5e-6    2.9e-4    0.45       0.23          0.95     2.2e-2
    far_eye           4.5e-7    1.7e-4    5.2e-5    1.2e-2    248        0.26          341      6.8e-2
    long_up           6.6e-7    2.0e-6    2.5e-6    3.1e-4    0.45       2.2e-4        0.95     6.3e-4
    near_degenerate   9.3e-5    1.5e-3    1.5e-3    1.6e-3    0.45       3.0e-4        0.95     9.8e-4
    close             3.2e-7    6.3e-5    6.3e-5    5.2e-5    1.8e-4     3.8e-2        2.8e-4   9.1e-2

so no fixed tolerance serves all of them; the bound follows the family (camera_reference.compare).
"""
import pytest
import torch

import camera_reference as cr

MARGIN = 10.0    # times the cut-off: a float32 length is within 1e-6 RELATIVE of the float64 one, so no flag can flip


@pytest.mark.parametrize("batch", [257, cr.SIZE])
@pytest.mark.parametrize("name", cr.FAMILIES)
def test_families_are_clear_of_the_degeneracy_cutoff(name, batch):
    cam = cr.family(name, batch)
    for dtype in (torch.float64, torch.float32):
        f_len, s_len = cr.lengths(cam, dtype)
        print("%-16s B %3d %s  min f_len %.3g  min s_len %.3g" % (name, batch, dtype, float(f_len.min()), float(s_len.min())))
        assert float(f_len.min()) > MARGIN * cr.CUTOFF and float(s_len.min()) > MARGIN * cr.CUTOFF
        assert int(cr.flags(cam, dtype).sum()) == 0
    for k in ("eye", "center", "up", "fov", "near", "far"):
        assert cam[k].dtype == torch.float32 and bool(torch.isfinite(cam[k]).all())
    assert float(cam["fov"].min()) >= 10.0 and float(cam["fov"].max()) <= 160.0
    assert float(cam["near"].min()) >= 0.01 and float((cam["far"] - cam["near"]).min()) >= 1.0 - 1e-6


def test_families_differ_where_they_say():
    plain = cr.family("plain", 64)
    assert float((cr.family("far_eye", 64)["eye"] / plain["eye"]).mean()) == pytest.approx(300.0, rel=1e-6)
    up_len = cr.family("long_up", cr.SIZE)["up"].norm(dim=1)
    assert float(up_len.min()) < 1e-2 and float(up_len.max()) > 1e2
    assert float(cr.lengths(cr.family("near_degenerate", 64))[1].max()) < 0.1
    assert float(cr.lengths(cr.family("close", 64))[0].max()) < 0.01
    assert torch.equal(cr.family("close", 64)["eye"], plain["eye"])   # the plain part is common


@pytest.mark.parametrize("name", cr.FAMILIES)
def test_truth_gradients_are_alive_and_the_yardstick_is_defined(name):
    cam, w, truth, r = cr.family_truth(name)
    print("%-16s r: %s" % (name, "  ".join("%s %.2g" % kv for kv in sorted(r.items()))))
    for k, t in truth.items():
        assert bool(torch.isfinite(t).all()), k
        per_camera = t.reshape(cr.SIZE, -1).abs().max(1).values
        assert float(per_camera.min()) > 0.0, (name, k)      # every camera: the bound is relative to it
        assert 0.0 < r[k] < float("inf"), (name, k, r[k])


@pytest.mark.parametrize("name", cr.FAMILIES)
def test_jacobian_reproduces_the_weighted_gradients(name):
    cam = cr.prefix(cr.family(name, 8), 8)
    w = cr.weights_for(8)
    truth, r = cr.evaluate(cam, w)
    J = cr.jacobian(*[cam[k] for k in ("eye", "center", "up", "fov", "near", "far")], cr.ASPECT)
    assert J.shape == (8, 16, 9) and J.dtype == torch.float64
    pulled = torch.einsum("bik,bi->bk", J, w.double().reshape(8, 16))
    # the same float64 derivative summed in another order: far inside the bound of a float32 evaluation (a wrong index
    # order in J would be off by the whole gradient)
    got = {k: pulled[:, 3 * i:3 * i + 3] for i, k in enumerate(cr.INPUTS)}
    over, ratios = cr.compare(name + " J^T w", got, truth, r, k=1)
    assert not over and max(ratios.values()) < 1, (over, ratios)

def test_float32_and_float64_agree_on_the_flags_of_an_edited_batch():
    for edit, bits in (("eye_is_center", 1), ("up_along_gaze", 2), ("nan_eye", 3), (None, 0)):
        cam = cr.degenerate_batch(edit)
        for dtype in (torch.float32, torch.float64):
            f = cr.flags(cam, dtype)
            assert int(f[300]) == bits and int(f.sum()) == bits, (edit, dtype)

