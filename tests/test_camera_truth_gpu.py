"""The camera kernels (csrc/mesh_ops.hip: k_camera_transforms, k_camera_transforms_backward) against a float64 truth.

tests/camera_reference.py holds the restatement, the five seeded camera families and the bound;
tests/test_camera_truth_host.py checks without a GPU that the families are fit to judge by.  Here every family runs
through _native.camera_transforms / camera_transforms_backward at B = 1, 7, 256, 257 and 600 (one thread per camera,
256 threads per block: a lone camera, a partly filled block, a full one, one camera in a second block, a partly
filled third), with random [B,4,4] upstream weights, and per tensor and camera

    |kernel - f64|[b]  <=  K * r * max|f64[b]|  +  1e-7 * max|f64|          (K = 8)

r being the float32 restatement's worst per-camera relative error over the family -- computed on the CPU from the
restatement alone.  Every run prints the kernel's worst per-camera relative error, r and their ratio.

MEASURED on the MI355X (ratio = kernel's worst per-camera relative error / r, at B = 600; the smaller batches are
prefixes and cannot exceed it; r is the yardstick of the host that ran the test and moves by up to 2x between CPUs):

    family            matrix  d eye   d center  d up        r (matrix .. d up)
    plain             0.73    0.67    2.75      0.66        5.3e-7  2.2e-6  2.5e-6  1.8e-4
    far_eye           1.23    1.64    1.00      2.16        4.5e-7  1.7e-4  5.2e-5  1.2e-2
    long_up           1.00    1.25    2.75      0.38        6.6e-7  2.0e-6  2.5e-6  1.4e-4
    near_degenerate   1.00    1.00    1.00      0.88        9.3e-5  1.5e-3  1.5e-3  1.7e-3
    close             1.36    0.98    0.98      0.88        3.2e-7  6.3e-5  6.3e-5  5.2e-5

The worst ratio is 2.75: no family needs more than K = 8.  The torch fall-back is at 0.02 .. 2.86 of r (d fov: 0.07 ..
1.17).  One-line mutations of k_camera_transforms_backward (not committed) -- gf += cross(up, gs_raw) dropped; the sign
of the dv[2][3] term of ge -- fail 25 and 24 of the 25 kernel cases here at 69 .. 8.5e5 and 2.7 .. 1.3e5 times the
allowance.

The first run found the flag word wrong for eye == center: 3 instead of 1 (the gaze is 0 / 0, |gaze x up| a NaN, and "not
greater than the cut-off" raised bit 1 whatever the up vector).  Fixed in k_camera_transforms: bit 1 is judged only on a
camera that has a gaze; a NaN input still raises both.

Flags: in a batch of 600 plain cameras, camera 300 alone is made degenerate -- eye == center (bit 0), up parallel to
the gaze (bit 1), a NaN eye component (both) -- and the launch returns exactly those bits, clip_space_transforms
raises the matching message, and the unedited batch returns 0.

Fall-back: a fov_y that requires grad takes the torch expression on the device (no kernel call), and its gradients to
eye, center, up and fov meet the same bound.
"""
import pytest
import torch

import camera_reference as cr
from pytorch_mesh_renderer_amd import _native
from pytorch_mesh_renderer_amd.common import camera_utils

pytestmark = pytest.mark.gpu

ORDER = ("eye", "center", "up", "fov", "near", "far")


@pytest.mark.parametrize("batch", [1, 7, 256, 257, 600])
@pytest.mark.parametrize("name", cr.FAMILIES)
def test_camera_kernels_against_the_float64_truth(device, name, batch):
    cam, weights, truth, r = cr.family_truth(name)
    args = [cam[k][:batch].contiguous().to(device) for k in ORDER]
    matrix, flags = _native.camera_transforms(*args, cr.ASPECT)
    assert int(flags.item()) == 0
    deye, dcenter, dup = _native.camera_transforms_backward(weights[:batch].contiguous().to(device), *args, cr.ASPECT)
    got = {"matrix": matrix, "eye": deye, "center": dcenter, "up": dup}
    for k, t in got.items():
        assert t.shape == truth[k][:batch].shape and t.dtype == torch.float32, k
    over, _ = cr.compare("%s B=%d" % (name, batch), got, truth, r, batch)
    assert not over, "\n".join(over)


@pytest.mark.parametrize("edit,bits,message", [("eye_is_center", 1, "eye and center are close"),
                                               ("up_along_gaze", 2, "up and gaze are too close"),
                                               ("nan_eye", 3, "eye and center are close"),
                                               (None, 0, None)])
def test_one_degenerate_camera_in_a_large_batch_raises_exactly_its_flags(device, edit, bits, message):
    cam = cr.degenerate_batch(edit)
    args = [cam[k].to(device) for k in ORDER]
    _, flags = _native.camera_transforms(*args, cr.ASPECT)
    assert int(flags.item()) == bits
    assert int(cr.flags(cam)[300]) == bits
    if message is None:
        assert camera_utils.clip_space_transforms(*args, cr.ASPECT, device).shape == (cr.SIZE, 4, 4)
    else:
        with pytest.raises(AssertionError, match=message):
            camera_utils.clip_space_transforms(*args, cr.ASPECT, device)


class _CountCalls:
    def __init__(self, name):
        self.name, self.calls = name, 0

    def __enter__(self):
        self.real = getattr(_native, self.name)

        def counted(*a, **k):
            self.calls += 1
            return self.real(*a, **k)
        setattr(_native, self.name, counted)
        return self

    def __exit__(self, *exc):
        setattr(_native, self.name, self.real)


@pytest.mark.parametrize("name", cr.FAMILIES)
def test_fov_gradient_takes_the_torch_expression_and_meets_the_same_bound(device, name):
    batch = 257
    cam, weights, truth, r = cr.family_truth(name, fov_grad=True)
    leaves = {k: cam[k][:batch].clone().to(device).requires_grad_(k in ("eye", "center", "up", "fov")) for k in ORDER}
    with _CountCalls("camera_transforms") as counter:
        m = camera_utils.clip_space_transforms(*[leaves[k] for k in ORDER], cr.ASPECT, device)
    assert counter.calls == 0
    (m * weights[:batch].to(device)).sum().backward()
    got = {"matrix": m, "eye": leaves["eye"].grad, "center": leaves["center"].grad, "up": leaves["up"].grad,
           "fov": leaves["fov"].grad}
    over, _ = cr.compare("%s fov fall-back" % name, got, truth, r, batch)
    assert not over, "\n".join(over)
    # and with the fov detached the same call is one kernel launch
    with _CountCalls("camera_transforms") as counter:
        camera_utils.clip_space_transforms(*[leaves[k].detach() for k in ORDER], cr.ASPECT, device)
    assert counter.calls == 1
